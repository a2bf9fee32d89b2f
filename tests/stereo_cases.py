"""Designed inputs for the sparse stereo rule (tests/stereo_restatement.py), shared by the CPU test of the restatement and the GPU tests of
the device kernel: small pairs whose answer is known without the restatement, and `shelf` pairs with the oracle's filtered corners and
the renderer's true depth.  Every case is dict(left, right, xyl, cam, baseline, rule, want): `want` the statuses the case is designed for
(None where the restatement is the only statement).  Made once per process, read-only.

A point of the left image's column x at disparity d is seen at the right image's column x - d: right[:, u] = left[:, u + d].

Test infrastructure only."""
import numpy as np

import stereo_restatement as sr
from oraclelib import TUM_CAM, trajectory_pose
import scene_cases as sc

W, H = 160, 120            # the small pairs: five pyramid levels (10 x 7 at level 4)
BASELINE = 0.11
SHELF_FRAMES = (0, 13, 26, 39)

_made = {}


def ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def case(left, right, xyl, want=None, cam=TUM_CAM, baseline=BASELINE, **rule):
    return dict(left=ro(left), right=ro(right), xyl=ro(np.asarray(xyl, np.int32).reshape(-1, 3)), cam=cam, baseline=baseline, rule=rule,
                want=None if want is None else np.asarray(want, np.uint8))


def restate(c):
    return sr.stereo_depth(c["left"], c["right"], c["xyl"], c["cam"], c["baseline"], **c["rule"])


def ramp(w=W, h=H):
    """L(x, y) = x + y // 2: every sample of a window differs from its neighbour at distance e by exactly |e|, so S(d) = 81 |d - d_true| s"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx + yy // 2).astype(np.uint8)


def texture(w, h, seed, smooth=True):
    """a smooth texture of full contrast (random sinusoids) or, smooth=False, independent noise"""
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.zeros((h, w))
    for _ in range(12):
        fx, fy = rng.uniform(-0.35, 0.35, 2)
        t += rng.uniform(0.5, 1.0) * np.sin(fx * xx + fy * yy + rng.uniform(0, 6.28))
    t = (t - t.min()) / (t.max() - t.min())
    return np.round(t * 255).astype(np.uint8)


def shifted(left, d, fill_seed=1):
    """the right image of a fronto-parallel scene at disparity d; the columns the left image does not cover are noise"""
    h, w = left.shape
    right = np.random.default_rng(fill_seed).integers(0, 256, (h, w)).astype(np.uint8)
    right[:, :w - d] = left[:, d:]
    return right


def inner_corners(levels, d_need, w=W, h=H, step=3):
    """corners of the given levels whose windows lie inside the image and whose range reaches past d_need"""
    out = []
    for l in levels:
        s = 1 << l
        for y in range(4, (h - 1) // s - 3, step):
            for x in range(4 + (d_need + s - 1) // s + 1, (w - 1) // s - 3, step):
                out.append((x, y, l))
    return out


def integer_shift_case(d=7):
    """the ramp shifted by d: every corner OK with d0 = d, delta exactly 0 (S- = S+ = 81 s), z = fx b / d"""
    left = ramp()
    xyl = inner_corners((0, 1, 2), d + 1)
    return case(left, shifted(left, d), xyl, np.zeros(len(xyl)))


def noise_shift_case(d=11):
    """independent noise shifted by d: S(d) = 0 and every other cost is large: OK with d0 = d"""
    left = texture(W, H, 20261101, smooth=False)
    xyl = inner_corners((0, 1, 2, 3), d + 1)
    return case(left, shifted(left, d), xyl, np.zeros(len(xyl)))


STEEP_FROM, STEEP_TO = 48, 111


def half_shift_case(d=9):
    """a steep ramp (4 gray levels a column between columns 48 and 111, flat beyond) shifted by d + 0.5: the mean of the shifts by d and
    d + 1, which is exact in 8 bits.  For a corner whose windows stay on the slope S(d) = S(d + 1) = 81 x 2, S(d - 1) = S(d + 2) = 81 x 6:
    the tie goes to d, the parabola puts the minimum at d + 0.5 exactly"""
    yy, xx = np.mgrid[0:H, 0:W]
    left = np.clip(4 * (xx - STEEP_FROM) + yy % 5, 0, 255).astype(np.uint8)
    a, b = shifted(left, d).astype(np.int32), shifted(left, d + 1).astype(np.int32)
    xyl = [(x, y, 0) for y in range(6, H - 6, 9) for x in range(STEEP_FROM + 7, STEEP_TO - 6, 4)]
    return case(left, ((a + b) // 2).astype(np.uint8), xyl, np.zeros(len(xyl)))


def constant_case():
    """a constant pair: every cost is equal, the tie rule makes the argmin the range's first disparity, an end: NOMATCH (never OK).  The
    same with a right image one gray level brighter."""
    left = np.full((H, W), 100, np.uint8)
    xyl = [(80, 60, 0), (40, 30, 1), (20, 15, 2)]
    return case(left, left.copy(), xyl, [sr.NOMATCH] * 3), case(left, left + 1, xyl, [sr.NOMATCH] * 3)


def periodic_case(period=8, d=10):
    """a texture of horizontal period 8, the right image shifted by 10 and one gray level brighter: S = 81 at d = 2, 10, 18, ...; d0 = 2
    and S2 = S(d0): AMBIGUOUS"""
    tile = texture(period, H, 20261103, smooth=False)
    left = np.tile(tile, (1, W // period))
    right = np.roll(left, -d, axis=1)          # (periodic: the roll is the shift)
    right = (right.astype(np.int32) + np.where(right < 255, 1, -1)).astype(np.uint8)
    xyl = [(80, 60, 0), (100, 30, 0), (50, 30, 1)]
    return case(left, right, xyl, [sr.AMBIGUOUS] * 3)


def outside_case():
    """X - 4 s in {-1, 0, 1}: OUTSIDE (the window leaves the image, or the range holds fewer than 3 disparities); X - 4 s in {2, 3}: a
    range of 3 and 4, whatever it finds it is not OUTSIDE; and windows that leave the image at the three other borders"""
    left = ramp()
    xyl, want = [], []
    for l in (0, 1, 2, 3):
        s = 1 << l
        if l == 0:
            for k in (-1, 0, 1, 2, 3):
                xyl.append((4 + k, 60, 0))
                want.append(sr.OUTSIDE if k < 2 else None)
        else:
            for x in (3, 4, 5):          # X - 4 s = -s, 0, s
                xyl.append((x, 60 >> l, l))
                want.append(sr.OUTSIDE if x < 5 else None)
        xb, yb = (W - 1) // s, (H - 1) // s
        xyl += [(xb - 3, 60 >> l, l), (80 >> l, 3, l), (80 >> l, yb - 3, l), (80 >> l, 0, l), (xb, yb, l), (0, 0, l)]
        want += [sr.OUTSIDE] * 6
        xyl += [((W - 1 - 4 * s) // s, 4, l)]      # the last window that fits the top right corner
        want.append(None)
    return case(left, shifted(left, 1), xyl), want


def range_end_case():
    """the ramp shifted by 7 searched up to 7: the best is the range's last disparity; shifted by 0: its first; shifted by 9 with a
    max_depth that starts the range at 9: its first again.  All NOMATCH"""
    left = ramp()
    xyl = inner_corners((0, 1), 12, step=7)
    n = len(xyl)
    fb = TUM_CAM[0] * BASELINE
    return [case(left, shifted(left, 7), xyl, [sr.NOMATCH] * n, max_disparity=7),
            case(left, left.copy(), xyl, [sr.NOMATCH] * n),
            case(left, shifted(left, 9), xyl, [sr.NOMATCH] * n, max_depth=fb / 9.5)]


def d_lo_case(d=12):
    """max_depth set so that the range starts at 5 > 0: the ramp shifted by 12 is found all the same, and the ramp shifted by 3 is not"""
    left = ramp()
    xyl = inner_corners((0, 1, 2), d + 1, step=5)
    fb = TUM_CAM[0] * BASELINE
    assert sr.call_range(TUM_CAM[0], sr.rule(BASELINE, max_depth=fb / 5.5))[1] == 5
    return (case(left, shifted(left, d), xyl, np.zeros(len(xyl)), max_depth=fb / 5.5),
            case(left, shifted(left, 3), xyl, [sr.NOMATCH] * len(xyl), max_depth=fb / 5.5))


EDGE_X, EDGE_NEAR, EDGE_FAR = 80, 5, 14


def edge_case():
    """the ramp seen at two depths: right[u] = left[u + 5] up to column EDGE_X - 5, left[u + 14] beyond — the left half of the window of
    a corner at column EDGE_X lies at disparity 5, its right half on the other surface.  The full window's best is a compromise (7) that
    the left half window's argmin (5) contradicts: EDGE.  Corners well to the left of the step are OK at disparity 5."""
    left = ramp()
    right = shifted(left, EDGE_FAR)
    right[:, :EDGE_X - EDGE_NEAR + 1] = left[:, EDGE_NEAR:EDGE_X + 1]
    xyl = [(EDGE_X, y, 0) for y in (20, 60, 100)] + [(EDGE_X - 30, y, 0) for y in (20, 60, 100)]
    return case(left, right, xyl, [sr.EDGE] * 3 + [sr.OK] * 3)


def designed_cases():
    if "designed" not in _made:
        out = {"integer": integer_shift_case(), "noise": noise_shift_case(), "half": half_shift_case(), "constant": constant_case()[0],
               "constant1": constant_case()[1], "periodic": periodic_case(), "outside": outside_case()[0], "edge": edge_case(),
               "dlo": d_lo_case()[0], "dlo_miss": d_lo_case()[1]}
        for k, c in enumerate(range_end_case()):
            out["end%d" % k] = c
        _made["designed"] = out
    return _made["designed"]


# ---- searched ranges around the lane rounds (64 lanes, at most 8 rounds) and the cap
RANGES = (3, 63, 64, 65, 128, 129, 512)
RANGE_W, RANGE_H = 640, 64


def range_case(n_range):
    """a 640 x 64 smooth texture shifted by about two thirds of the range, searched over exactly n_range disparities (d_lo = 0,
    max_disparity = n_range - 1, min_depth small enough not to matter): corners of levels 0 - 3 whose own limit X - 4 s lies beyond it,
    and two whose limit cuts the range short"""
    key = ("range", n_range)
    if key not in _made:
        d = max(1, (2 * n_range) // 3)
        left = texture(RANGE_W, RANGE_H, 20261110 + n_range)
        xyl = []
        for l in (0, 1, 2, 3):
            s = 1 << l
            x_min = (n_range - 1 + 4 * s + s - 1) // s
            xs = sorted(set(np.linspace(x_min, (RANGE_W - 1) // s - 4, 5).astype(int)))
            xyl += [(int(x), y, l) for x in xs for y in (4, (RANGE_H - 1) // s - 4) if x * s - 4 * s >= n_range - 1]
        xyl += [(max(5, (n_range // 2) + 4), 20, 0), (6, 30, 0)]
        _made[key] = case(left, shifted(left, min(d, RANGE_W - 1)), xyl, max_disparity=max(n_range - 1, 1), min_depth=0.01)
    return _made[key]


# ---- `shelf` pairs
def filtered_corners(orc, img):
    corners = orc.detect_pyramid(img)
    return corners[orc.filter_corners(img, corners)]


def right_pose(T_cw, baseline):
    """the right camera: its centre is the left one's plus `baseline` along the left camera's x axis, the same orientation, so
    t_right = t_left - (baseline, 0, 0)"""
    T = np.array(T_cw, np.float64)
    T[4] -= baseline
    return T


def shelf_pair(orc, k, baseline=BASELINE, i=0):
    """frame k of tracker i's `shelf` trajectory as a stereo pair, no lens: the oracle's filtered corners of the left image and the
    renderer's true depth of the left view -> (case, depth float32 [h][w])"""
    key = ("shelf", i, k, baseline)
    if key not in _made:
        ss = sc.scene_synth()
        T = trajectory_pose(orc, k, sc.tracker_twist(i))
        left, depth, _ = ss.render(ss.scene(T, preset="shelf", seed=sc.SEED + i, frame_id=k))
        right = ss.render(ss.scene(right_pose(T, baseline), preset="shelf", seed=sc.SEED + i, frame_id=k), truth=False)
        _made[key] = (case(left, right, filtered_corners(orc, left), baseline=baseline), ro(depth))
    return _made[key]


def true_disparity(c, depth):
    """fx b / the renderer's depth at every corner's level-0 pixel"""
    xyl = c["xyl"].astype(np.int64)
    s = 1 << xyl[:, 2]
    return c["cam"][0] * c["baseline"] / depth[xyl[:, 1] * s, xyl[:, 0] * s].astype(np.float64)
