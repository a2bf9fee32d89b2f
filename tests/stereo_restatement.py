"""The sparse stereo rule (sdvl_stereo_depth, include/sdvl_hip.h) restated in plain numpy: integer SADs, a float64 tail.  It is the
SPECIFICATION of the device kernel stereo_depth (slam-sdvl_amd/csrc/sdvl_stereo.hip).  The rule is this project's own; nothing here is
taken from the reference or from OpenCV.

A corner (x, y, l) in level coordinates has the level-0 pixel (X, Y) = (x s, y s), s = 1 << l.  Both images are 8-bit gray of one size,
rectified so that rows correspond; the right camera sits `baseline` metres along the left camera's x axis, so a point at depth z has the
disparity fx baseline / z and is seen in the right image at column X - d.  Per corner:
  window   the 9 x 9 samples at (X + i s, Y + j s), i, j in -4 .. 4, of level 0 of both images
  range    d_lo = floor(fx b / max_depth) if max_depth > 0 else 0;  d_hi = min(max_disparity, floor(fx b / min_depth), X - 4 s)
  cost     S(d) = sum |L - R| over the 81 samples; d0 its argmin, ties to the smallest d; four half-window costs from the same absolute
           differences: sample columns 0 - 4, columns 4 - 8, rows 0 - 4, rows 4 - 8
  status   the first that applies of OUTSIDE (the left window leaves the image, or fewer than 3 disparities in the range), NOMATCH
           (S(d0) > 81 max_sad, or d0 is an end of the range), AMBIGUOUS (100 S(d0) > uniqueness S2, S2 = min S(d) over |d - d0| > 1, when
           there is such a d), EDGE (some half window's argmin, same tie rule, differs from d0 by more than 1), else OK
  result   delta = 0.5 (S- - S+) / (S- - 2 S0 + S+) when the denominator is positive, else 0; disparity = d0 + delta; z = fx b / disparity;
           both 0 unless OK.  The operation order is the one written in `parabola` below; the device code is built without contraction.

Test infrastructure only."""
import math

import numpy as np

OK, NOMATCH, AMBIGUOUS, EDGE, OUTSIDE = 0, 1, 2, 3, 4
STATUS_NAMES = ("OK", "NOMATCH", "AMBIGUOUS", "EDGE", "OUTSIDE")
DEFAULTS = dict(min_depth=0.3, max_depth=0.0, max_disparity=192, max_sad=20, uniqueness=80)
HALF = 4                 # the window is 2 HALF + 1 samples a side
MAX_DISPARITY = 511
MAX_LEVELS = 8           # SDVL_MAX_LEVELS


class Refused(ValueError):
    """what sdvl_stereo_depth answers with SDVL_ERR_INVALID and a message"""


def rule(baseline, **kw):
    """the rule's numbers; a field given as 0 takes its default, as in sdvl_stereo_params.  Refuses what the entry refuses."""
    r = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in r:
            raise Refused("unknown rule field %s" % k)
        if v != 0:
            r[k] = v
    b = float(baseline)
    if not (math.isfinite(b) and b > 0.0):
        raise Refused("baseline is not a positive finite number")
    if not (r["min_depth"] > 0.0 and math.isfinite(r["min_depth"])) or not (r["max_depth"] >= 0.0 and math.isfinite(r["max_depth"])):
        raise Refused("min_depth / max_depth negative or not finite")
    if not 0 < r["max_disparity"] <= MAX_DISPARITY:
        raise Refused("max_disparity outside 1 .. 511")
    if not 1 <= r["uniqueness"] <= 100:
        raise Refused("uniqueness outside 1 .. 100")
    if r["max_sad"] < 0 or r["max_sad"] > 255:
        raise Refused("max_sad outside 1 .. 255")
    r["baseline"] = b
    return r


def call_range(fx, r):
    """-> (fb, d_lo, d_cap): fx b, and the two ends of the range that do not depend on the corner.  floor() of a quotient beyond the
    largest disparity is cut there first (the device converts to int)"""
    fb = np.float64(fx) * np.float64(r["baseline"])
    big = np.float64(MAX_DISPARITY + 1)
    d_lo = int(min(np.floor(fb / np.float64(r["max_depth"])), big)) if r["max_depth"] > 0 else 0
    d_cap = min(int(r["max_disparity"]), int(min(np.floor(fb / np.float64(r["min_depth"])), big)))
    return fb, d_lo, d_cap


def parabola(s_minus, s0, s_plus):
    """the sub-pixel offset of the minimum of the parabola through three integer costs, float64, in this operation order"""
    den = int(s_minus) - 2 * int(s0) + int(s_plus)
    if den <= 0:
        return np.float64(0.0)
    return np.float64(0.5) * np.float64(int(s_minus) - int(s_plus)) / np.float64(den)


def costs(left, right, X, Y, s, d_lo, d_hi):
    """-> int64 [5][d_hi - d_lo + 1]: the full cost and the four half-window costs (columns 0-4, columns 4-8, rows 0-4, rows 4-8) of every
    disparity of the range.  The windows lie inside both images."""
    off = np.arange(-HALF, HALF + 1) * s
    L = left[np.ix_(Y + off, X + off)].astype(np.int64)
    out = np.zeros((5, d_hi - d_lo + 1), np.int64)
    for k, d in enumerate(range(d_lo, d_hi + 1)):
        a = np.abs(L - right[np.ix_(Y + off, X - d + off)].astype(np.int64))
        out[:, k] = (a.sum(), a[:, :HALF + 1].sum(), a[:, HALF:].sum(), a[:HALF + 1, :].sum(), a[HALF:, :].sum())
    return out


def check_inputs(left, right, xyl, levels):
    left, right = np.asarray(left), np.asarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2 or left.shape != right.shape:
        raise Refused("the images are not 8-bit gray of one size")
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3)
    if len(xyl) and not ((xyl[:, 2] >= 0).all() and (xyl[:, 2] < levels).all()):
        raise Refused("a corner's level lies outside the pyramid")
    return left, right, xyl


def stereo_depth(left, right, xyl, cam, baseline, dist=None, levels=5, **kw):
    """left, right: [h, w] uint8; xyl [n][3]; cam = (fx, fy, u0, v0); levels: the depth of the left frame's pyramid
    -> dict(z float64 [n], disparity float64 [n], status uint8 [n], d0 int32 [n] (-1 where no cost was taken), s0 int64 [n])"""
    if dist is not None and float(dist[0]) != 0.0:
        raise Refused("a lens: rectified pairs only")
    r = rule(baseline, **kw)
    left, right, xyl = check_inputs(left, right, xyl, levels)
    h, w = left.shape
    fb, d_lo, d_cap = call_range(cam[0], r)
    n = len(xyl)
    z, disp, status = np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)
    d0s, s0s = np.full(n, -1, np.int32), np.zeros(n, np.int64)
    for i in range(n):
        x, y, l = [int(v) for v in xyl[i]]
        s = 1 << l
        X, Y = x * s, y * s
        if x < 0 or y < 0 or X - HALF * s < 0 or X + HALF * s >= w or Y - HALF * s < 0 or Y + HALF * s >= h:
            status[i] = OUTSIDE
            continue
        d_hi = min(d_cap, X - HALF * s)
        if d_hi - d_lo + 1 < 3:
            status[i] = OUTSIDE
            continue
        c = costs(left, right, X, Y, s, d_lo, d_hi)
        best = [int(np.argmin(c[k])) for k in range(5)]       # (numpy's argmin is the first of equal minima: the smallest d)
        i0 = best[0]
        S0 = int(c[0, i0])
        d0s[i], s0s[i] = d_lo + i0, S0
        if S0 > 81 * r["max_sad"] or i0 == 0 or i0 == d_hi - d_lo:
            status[i] = NOMATCH
            continue
        far = np.abs(np.arange(d_hi - d_lo + 1) - i0) > 1
        if far.any() and 100 * S0 > r["uniqueness"] * int(c[0, far].min()):
            status[i] = AMBIGUOUS
            continue
        if any(abs(b - i0) > 1 for b in best[1:]):
            status[i] = EDGE
            continue
        disp[i] = np.float64(d_lo + i0) + parabola(c[0, i0 - 1], S0, c[0, i0 + 1])
        z[i] = fb / disp[i]
    return dict(z=z, disparity=disp, status=status, d0=d0s, s0=s0s)


def stereo_jobs(jobs, xyl, cam, baseline, dist=None, **kw):
    """the entry's call: jobs = [(left, right, c_begin, c_end), ...] over one corner list; a corner no job names comes back NOMATCH.
    -> (z, disparity, status, ok per job)"""
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3)
    n = len(xyl)
    rule(baseline, **kw)
    named = np.zeros(n, bool)
    for _, _, b, e in jobs:
        if not 0 <= b <= e <= n:
            raise Refused("corner range outside the corner list")
        if named[b:e].any():
            raise Refused("corner ranges overlap")
        named[b:e] = True
    z, disp, status, ok = np.zeros(n), np.zeros(n), np.full(n, NOMATCH, np.uint8), []
    for left, right, b, e in jobs:
        out = stereo_depth(left, right, xyl[b:e], cam, baseline, dist, **kw)
        z[b:e], disp[b:e], status[b:e] = out["z"], out["disparity"], out["status"]
        ok.append(int((out["status"] == OK).sum()))
    return z, disp, status, np.array(ok, np.int32)


def d0_of(disparity):
    """the integer disparity behind an OK corner's result: delta lies in (-0.5, 0.5] (a tie with d0 - 1 would have made that the argmin)"""
    return np.ceil(np.asarray(disparity) - 0.5).astype(np.int32)
