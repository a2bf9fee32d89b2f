"""The depth-seeding rule (sdvl_depth_seed, include/sdvl_hip.h) restated in plain numpy, FP64: the SPECIFICATION of the device kernel
depth_seed (slam-sdvl_amd/csrc/sdvl_depth.hip).  The rule is this project's own; nothing here is taken from the reference.

A corner (x, y, l) in level coordinates has the level-0 pixel (X, Y) = (x s, y s), s = 1 << l.  The depth image lies on the pixel grid of
the camera image as delivered (the raw grid).  With a lens the gray image was undistorted, so the centre sample is the raw pixel the
corner's ray lands on: the forward model of cv::undistort, in the operation order written below (numpy does not contract a * b + c, and
the device code is built without contraction: the same doubles, ties included).  The window is the nine samples at (cx + i s, cy + j s).

Test infrastructure only."""
import numpy as np

OK, HOLE, FEW, EDGE, OUTSIDE = 0, 1, 2, 3, 4
STATUS_NAMES = ("OK", "HOLE", "FEW", "EDGE", "OUTSIDE")
DEFAULTS = dict(min_depth=0.05, max_depth=0.0, edge_ratio=0.05, min_valid=6)


def rule(**kw):
    """the rule's four numbers; a field given as 0 takes its default, as in sdvl_depth_seed_params"""
    r = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in r, k
        if v != 0:
            r[k] = v
    return r


def centre_pixels(xyl, cam, dist=None):
    """-> (fu, fv) float64 [n]: the centre sample's column and row BEFORE the range test (whole numbers, or NaN / inf).
    cam = (fx, fy, u0, v0); dist = (k1, k2, p1, p2, k3), None or dist[0] == 0: no lens"""
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3)
    s = (1 << xyl[:, 2]).astype(np.float64)
    X, Y = xyl[:, 0].astype(np.float64) * s, xyl[:, 1].astype(np.float64) * s
    if dist is None or float(dist[0]) == 0.0:
        return X, Y
    fx, fy, u0, v0 = [np.float64(c) for c in cam]
    k1, k2, p1, p2, k3 = [np.float64(d) for d in dist]
    with np.errstate(all="ignore"):
        x, y = (X - u0) / fx, (Y - v0) / fy
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
        v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
        return np.floor(u + 0.5), np.floor(v + 0.5)


def metres(depth, scale=1.0):
    """the samples of a depth image as float64 metres: float32 as they are, uint16 times `scale` (one multiplication, as the device does)"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return depth.astype(np.float64) * np.float64(scale)
    assert depth.dtype == np.float32, depth.dtype
    return depth.astype(np.float64)


def valid(z, r):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0.0) & (z >= r["min_depth"]) & ((r["max_depth"] <= 0.0) | (z <= r["max_depth"]))


def depth_seed(depth, xyl, cam, dist=None, scale=1.0, **kw):
    """depth: [h, w] float32 (metres) or uint16 (units of `scale` metres) -> (z float64 [n], status uint8 [n], ranges float64 [n]: max - min
    over the valid samples relative to the centre's depth, NaN where the centre is not valid)"""
    r = rule(**kw)
    Z = metres(depth, scale)
    h, w = Z.shape
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3)
    n = len(xyl)
    fu, fv = centre_pixels(xyl, cam, dist)
    z, status, rel = np.zeros(n), np.zeros(n, np.uint8), np.full(n, np.nan)
    for i in range(n):
        if not (fu[i] >= 0 and fu[i] < w and fv[i] >= 0 and fv[i] < h):
            status[i] = OUTSIDE
            continue
        cx, cy, s = int(fu[i]), int(fv[i]), 1 << int(xyl[i, 2])
        zc = Z[cy, cx]
        if not valid(zc, r):
            status[i] = HOLE
            continue
        win = []
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                sx, sy = cx + k * s, cy + j * s
                if 0 <= sx < w and 0 <= sy < h and valid(Z[sy, sx], r):
                    win.append(Z[sy, sx])
        rel[i] = (max(win) - min(win)) / zc
        if len(win) < r["min_valid"]:
            status[i] = FEW
        elif max(win) - min(win) > r["edge_ratio"] * zc:
            status[i] = EDGE
        else:
            z[i] = zc
    return z, status, rel
