"""The cases of tests/test_gpu_stereo_lookup.py, shared with tests/test_stereo_lookup_restatement_cpu.py: positions for the stereo lookup
(tests/stereo_lookup_restatement.py) and candidates for the depth filter fed by it.  The pairs are stereo_cases' own, imported and not
edited.

Positions.  A level-l corner (x, y) of a designed pair becomes the position (x s + f_x, y s + f_y), |f| < 0.5: the lookup's answer is then
the corner's, which the restatement of sdvl_stereo_depth gives without this file.  The centre rule has cases of its own.  `shelf` corners
are displaced by a whole number of pixels below the stride too, so that the centre leaves the level's grid.

Candidates.  As depth_measure_cases builds them: the found pixel px and the depth z the matcher gives at its centre make
P_c = unproject(px) z / unproject(px).z, the current pose takes it to the world, and the candidate's bearing is the direction of that point
from the reference camera.  The pairs are 160 x 120 with the TUM camera's focal length, so a disparity of 7 is a depth of 8.1 m.

Test infrastructure only."""
import math

import numpy as np

import depth_cases as dcs
import depth_measure_cases as dmc
import depth_restatement as dr
import stereo_cases as stc
import stereo_lookup_restatement as sl
import stereo_restatement as sr
from depth_restatement import CONVERGED, DELETED, NOT_FOUND, SKIPPED, UPDATED
from oraclelib import TUM_CAM

W, H = stc.W, stc.H
CAM = dict(width=float(W), height=float(H), fx=float(TUM_CAM[0]), fy=float(TUM_CAM[1]), u0=float(TUM_CAM[2]), v0=float(TUM_CAM[3]))
PARAMS = dict(px_error_angle=dr.pixel_error_angle(CAM["fx"]), min_depth=0.25, scale_min_dist=0.25, max_failed=15)
SIGMA = 0.4                 # explicit: no test rests on the default
JITTER_SEED = 20261121

_made = {}


# ---------------------------------------------------------------------------------------------------- positions
def jitter(n, seed=JITTER_SEED):
    """n fixed pseudo-random offsets in (-0.5, 0.5) x (-0.5, 0.5), both signs and both sides of every quarter"""
    f = np.random.default_rng(seed).uniform(-0.499, 0.499, (n, 2))
    f.setflags(write=False)
    return f


def positions_of(c, seed=JITTER_SEED):
    """the corners of a stereo case as jittered level-0 positions -> (px [n][2], levels [n])"""
    xyl = c["xyl"].astype(np.int64)
    s = (1 << xyl[:, 2]).astype(np.float64)
    px = np.stack([xyl[:, 0] * s, xyl[:, 1] * s], 1) + jitter(len(xyl), seed + len(xyl))
    return stc.ro(px), stc.ro(xyl[:, 2].astype(np.int32))


def centre_cases():
    """-> (pair case, px, levels, want): want[i] a status, None where the restatement alone says, or ("as", x, y, l): the bits of that corner.
    The ramp shifted by 7: every centre whose window and range fit is OK at disparity 7"""
    c = stc.designed_cases()["integer"]
    px, lv, want = [], [], []

    def add(p, l, w):
        px.append(p); lv.append(l); want.append(w)

    add((80.5, 60.0), 0, ("as", 81, 60, 0))            # a fraction of exactly 0.5 goes up
    add((80.0, 59.5), 0, ("as", 80, 60, 0))
    add((79.5, 59.5), 0, ("as", 80, 60, 0))
    add((80.49999, 60.49999), 0, ("as", 80, 60, 0))
    add((81.0 - 2 ** -40, 60.0), 0, ("as", 81, 60, 0))  # above the half by less than anything a float32 would keep
    add((-0.6, 60.0), 0, sr.OUTSIDE)                   # a negative centre
    add((-3.0, -3.0), 1, sr.OUTSIDE)
    add((-0.4, 60.0), 0, sr.OUTSIDE)                   # rounds to column 0: inside the image, the window is not
    add((float("nan"), 60.0), 0, sr.OUTSIDE)
    add((80.0, float("nan")), 2, sr.OUTSIDE)
    add((float("inf"), 60.0), 0, sr.OUTSIDE)
    add((80.0, float("-inf")), 1, sr.OUTSIDE)
    add((1e300, 1e300), 0, sr.OUTSIDE)
    for X in (61, 63, 65, 67):                         # level 2, odd centres: no multiple of the stride
        add((X + 0.2, 57.0 - 0.3), 2, sr.OK)
    add((70.3, 51.2), 3, sr.OK)                        # level 3 off its grid
    for l in (0, 1, 2, 3):                             # a window touching each border: the last centre that fits, and one pixel further
        s = 1 << l
        lo_x = 4 * s + 9                               # the range must reach past the shift of 7: X - 4 s >= 8, and one more for the parabola
        add((lo_x, 60.0), l, sr.OK)
        add((4 * s - 1, 60.0), l, sr.OUTSIDE)          # left border
        add((W - 1 - 4 * s, 60.0), l, None)            # right border: the last that fits (not OUTSIDE)
        add((W - 4 * s, 60.0), l, sr.OUTSIDE)
        add((80.0, 4 * s), l, sr.OK)                   # top
        add((80.0, 4 * s - 1), l, sr.OUTSIDE)
        add((80.0, H - 1 - 4 * s), l, sr.OK)           # bottom
        add((80.0, H - 4 * s), l, sr.OUTSIDE)
    add((80.0, 60.0), 4, sr.OUTSIDE)                   # level 4 on 160 x 120: the window is 129 pixels tall
    return c, stc.ro(np.array(px, np.float64)), stc.ro(np.array(lv, np.int32)), want


def shelf_jittered(orc, k):
    """`shelf` frame k: the filtered corners displaced by a fixed pseudo-random offset below the stride — a whole number of pixels in
    -(s // 2) .. s // 2 plus a fraction in (-0.5, 0.5) -> (pair case, depth, px, levels, rounded centres int64 [n][2])"""
    key = ("shelf", k)
    if key not in _made:
        c, depth = stc.shelf_pair(orc, k)
        xyl = c["xyl"].astype(np.int64)
        n = len(xyl)
        s = 1 << xyl[:, 2]
        rng = np.random.default_rng(JITTER_SEED + 1000 + k)
        whole = np.stack([rng.integers(-(s // 2), s // 2 + 1), rng.integers(-(s // 2), s // 2 + 1)], 1)
        px = np.stack([xyl[:, 0] * s, xyl[:, 1] * s], 1) + whole + jitter(n, JITTER_SEED + 2000 + k)
        centres = np.floor(px + 0.5).astype(np.int64)
        _made[key] = (c, depth, stc.ro(px), stc.ro(xyl[:, 2].astype(np.int32)), stc.ro(centres))
    return _made[key]


def true_disparity_at(c, depth, centres):
    """fx b / the renderer's depth at the rounded centre (NaN off the image)"""
    h, w = depth.shape
    inside = (centres[:, 0] >= 0) & (centres[:, 0] < w) & (centres[:, 1] >= 0) & (centres[:, 1] < h)
    out = np.full(len(centres), np.nan)
    out[inside] = c["cam"][0] * c["baseline"] / depth[centres[inside, 1], centres[inside, 0]].astype(np.float64)
    return out


# ---------------------------------------------------------------------------------------------------- candidates of the filter
PAIRS = ("integer", "noise", "constant", "periodic", "edge", "dlo")


def pair(name):
    c = stc.designed_cases()[name]
    return c["left"], c["right"]


def measured_geometry(px, z, cur_pose, ref_pose=None):
    """depth_measure_cases.measured_geometry on this file's camera"""
    ref_pose = dcs.pose_of(dmc.REF_Q, dmc.REF_C) if ref_pose is None else ref_pose
    v = dr.unproject(CAM, px)
    k = z / v[2]
    P = dr.se3_apply(dr.se3_inverse(cur_pose), (v[0] * k, v[1] * k, v[2] * k))
    p_r = dr.se3_apply(ref_pose, P)
    rng = dr.norm3(p_r)
    return dict(cur_pose=cur_pose, ref_pose=ref_pose, bearing=(p_r[0] / rng, p_r[1] / rng, p_r[2] / rng), range=rng, P=P)


def matched(pair_name, px, level, rule=None):
    """-> (status, disparity, z) of the restatement's lookup on the pair"""
    left, right = pair(pair_name)
    return sl.lookup(np.asarray(left), np.asarray(right), px, level, TUM_CAM, stc.BASELINE, **(rule or {}))


def case(name, purpose, pair_name, px, level, st, k=0, found=True, rule=None, params=PARAMS, sigma=SIGMA, group="plain", z_for_geometry=None,
         baseline_cams=0.35, flip=False, **want):
    z = z_for_geometry
    if z is None:
        z = matched(pair_name, px, level, rule)[2] if pair_name is not None else 0.0
        z = z if z > 0 else 6.0
    geo = measured_geometry(px, z, dmc.cur_pose_of(k, baseline_cams))
    bearing = tuple(-c for c in geo["bearing"]) if flip else geo["bearing"]
    return dict(name=name, purpose=purpose, cur_pose=geo["cur_pose"], ref_pose=geo["ref_pose"], bearing=bearing, found=found, px=tuple(px), level=level,
                state=st, params=params, cam=CAM, pair=pair_name, baseline=stc.BASELINE, disparity_sigma=sigma, rule=rule or {}, group=group,
                range=geo["range"], want=want)


def inputs(c):
    return dict(cur_pose=c["cur_pose"], ref_pose=c["ref_pose"], bearing=c["bearing"], found=c["found"], px=c["px"], level=c["level"], cam=c["cam"],
                state=c["state"], params=c["params"], pair=None if c["pair"] is None else pair(c["pair"]), baseline=c["baseline"],
                disparity_sigma=c["disparity_sigma"], rule=c["rule"])


def triangulated_inputs(c):
    return dict(cur_pose=c["cur_pose"], ref_pose=c["ref_pose"], bearing=c["bearing"], found=c["found"], px=c["px"], cam=c["cam"], state=c["state"],
                params=c["params"])


S = dcs.state


def _ok_cases():
    out = []
    grid = [  # pair, px, level, k, rho factor, sigma2, a, b, z_range, n_failed
        ("integer", (80.3, 59.6), 0, 0, 1.10, 1.0, 10.0, 10.0, 6.0, 0),
        ("integer", (90.6, 40.7), 0, 1, 0.90, 0.05, 12.0, 9.0, 6.0, 3),
        ("integer", (75.5, 33.5), 0, 2, 1.02, 1e-3, 40.0, 3.0, 2.5, 1),        # both coordinates on the half: rounded up
        ("integer", (100.49, 62.51), 1, 3, 0.97, 1e-2, 25.0, 30.0, 6.0, 0),
        ("integer", (85.2, 57.4), 2, 4, 1.30, 1.0, 1.0, 1.0, 6.0, 7),          # level 2, the centre (85, 57) off the grid
        ("noise", (120.4, 60.2), 3, 5, 0.75, 0.3, 10.0, 14.0, 6.0, 0),         # level 3: a parabola that is not flat
        ("noise", (62.2, 83.9), 1, 6, 1.00, 1e-6, 300.0, 1.0, 2.5, 2),
        ("noise", (117.8, 22.1), 0, 7, 1.05, 1e-4, 150.0, 150.0, 6.0, 0),
        ("dlo", (99.7, 71.2), 1, 2, 0.95, 0.02, 14.0, 10.5, 6.0, 0),
    ]
    for i, (pn, px, level, k, fac, sigma2, a, b, z_range, nf) in enumerate(grid):
        rule = dict(stc.designed_cases()[pn]["rule"])
        z = matched(pn, px, level, rule)[2]
        assert z > 0, (pn, px, level)
        geo = measured_geometry(px, z, dmc.cur_pose_of(k))
        st = S(fac / geo["range"], sigma2=sigma2, a=a, b=b, z_range=z_range, depth_mean=5.0, n_failed=nf)
        out.append(case("ok-%02d-%s-level%d" % (i, pn, level), "a measured update on level %d, rho %.2f of the truth, sigma2 %.1g" % (level, fac, sigma2), pn,
                        px, level, st, k=k, rule=rule, group="plain" if not rule else "dlo", updated=True, exact_range=True, status=sr.OK))
    px = (89.7, 46.2)
    geo = measured_geometry(px, matched("integer", px, 0)[2], dmc.cur_pose_of(2))
    out.append(case("ok-converges", "a narrow prior at the measured range: l < 0.1 after the update", "integer", px, 0,
                    S(1.0 / geo["range"], sigma2=1e-7, a=30.0, b=8.0, depth_mean=5.0, n_failed=2), k=2, outcome=CONVERGED, exact_range=True, status=sr.OK))
    out.append(case("ok-wide-stays", "the seed state at the measured range: one update does not converge", "integer", px, 0,
                    S(1.0 / geo["range"], depth_mean=5.0), k=2, outcome=UPDATED, exact_range=True, status=sr.OK))
    fixed_at = (0.123, -4.5, 7.25)
    out.append(case("ok-fixed", "fixed = 1: CONVERGED whatever l is, the position is state.position", "integer", px, 1,
                    S(1.2 / geo["range"], sigma2=0.5, position=fixed_at, fixed=1, depth_mean=5.0), k=2, outcome=CONVERGED, position=fixed_at, status=sr.OK))
    out.append(case("ok-no-parallax", "the current camera 0.1 mm beside the reference one: no triangulation to guard, the update runs", "integer", (80.3, 59.6), 0,
                    S(1.1 / 8.0, sigma2=0.2, depth_mean=5.0), k=1, baseline_cams=1e-4, updated=True, exact_range=True, status=sr.OK))
    # the default sigma, and a sigma of its own, each a call of its own
    out.append(case("ok-sigma-default", "disparity_sigma 0: 0.25 px", "integer", (80.3, 59.6), 0, S(1.1 / 8.0, sigma2=0.2, depth_mean=5.0), k=1, sigma=0.0,
                    group="sigma0", updated=True, status=sr.OK))
    out.append(case("ok-sigma-small", "disparity_sigma 0.05 px", "integer", (80.3, 59.6), 0, S(1.1 / 8.0, sigma2=0.2, depth_mean=5.0), k=1, sigma=0.05,
                    group="sigma005", updated=True, status=sr.OK))
    return out


def _skipped_cases():
    out = []
    px = (80.3, 59.6)
    geo = measured_geometry(px, matched("integer", px, 0)[2], dmc.cur_pose_of(1))
    out.append(case("skip-depth_mean", "range %.3g < depth_mean 40 x 0.25: SKIPPED" % geo["range"], "integer", px, 0,
                    S(1.0 / geo["range"], sigma2=0.1, depth_mean=40.0), k=1, outcome=SKIPPED, status=sr.OK))
    out.append(case("skip-min_depth", "range %.3g < min_depth 20: SKIPPED" % geo["range"], "integer", px, 0, S(1.0 / geo["range"], sigma2=0.1, depth_mean=5.0),
                    k=1, params=dict(PARAMS, min_depth=20.0), group="min_depth20", outcome=SKIPPED, status=sr.OK))
    out.append(case("skip-negative-range", "the bearing reversed: the range is not positive, SKIPPED before the minimum-depth tests", "integer", px, 0,
                    S(1.0 / geo["range"], sigma2=0.1, depth_mean=-40.0), k=1, flip=True, params=dict(PARAMS, min_depth=-10.0), group="min_depth-10",
                    outcome=SKIPPED, status=sr.OK))
    return out


def _fallback_cases():
    """status not OK, or no pair: the triangulated update of depth_restatement on a geometry that triangulates"""
    out = []
    st = S(1.0 / 5.8, sigma2=0.05, a=11.0, b=12.0, depth_mean=5.0, n_failed=4)
    out.append(case("nomatch-constant", "a constant pair: every cost equal, the argmin an end of the range: NOMATCH", "constant", (80.3, 59.6), 0, st, k=1,
                    status=sr.NOMATCH))
    out.append(case("nomatch-level1", "the same on level 1", "constant", (80.7, 60.4), 1, st, k=2, status=sr.NOMATCH))
    out.append(case("ambiguous", "a texture of period 8: AMBIGUOUS", "periodic", (80.2, 59.8), 0, st, k=3, status=sr.AMBIGUOUS))
    out.append(case("edge", "a window on two depths: EDGE", "edge", (stc.EDGE_X + 0.3, 59.7), 0, st, k=4, status=sr.EDGE))
    out.append(case("edge-left-of-it", "thirty columns to the left of the step: the window stays on one surface", "edge", (stc.EDGE_X - 30 + 0.3, 59.7), 0, st, k=4,
                    updated=True, status=sr.OK))
    out.append(case("outside-right", "px 159.7 rounds to column 160: OUTSIDE", "integer", (159.7, 60.2), 0, st, k=2, status=sr.OUTSIDE))
    out.append(case("outside-window", "the centre is on the image, its level-2 window is not: OUTSIDE", "integer", (150.2, 60.2), 2, st, k=2, status=sr.OUTSIDE))
    out.append(case("outside-level4", "level 4 on 160 x 120: OUTSIDE", "integer", (80.2, 60.2), 4, st, k=2, status=sr.OUTSIDE))
    out.append(case("no-job", "a hit whose request is in no job: nothing is matched", None, (80.3, 59.6), 0, st, k=1, status=sl.NO_LOOKUP))
    out.append(case("no-job-level3", "the same on level 3", None, (70.1, 49.3), 3, st, k=5, status=sl.NO_LOOKUP))
    for nf in (3, 15):
        gone = nf + 1 > 15
        out.append(case("miss-n_failed-%d" % nf, "Unpromote from n_failed = %d: %s" % (nf, "deleted" if gone else "kept"), "integer", (80.3, 59.6), 0,
                        S(0.2, sigma2=0.04, a=12.5, b=7.25, cos_alpha=0.99, last_distance=2.1, n_failed=nf), k=1, found=False,
                        outcome=NOT_FOUND | (DELETED if gone else 0), status=sl.NO_LOOKUP))
    return out


def all_cases():
    if "cases" not in _made:
        _made["cases"] = _ok_cases() + _skipped_cases() + _fallback_cases()
        names = [c["name"] for c in _made["cases"]]
        assert len(set(names)) == len(names)
    return _made["cases"]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def groups():
    out = {}
    for c in all_cases():
        out.setdefault(c["group"], []).append(c)
    return out


_TOL = {}


def expected(c):
    """-> (the restatement's result, the bound per float output), computed once per case"""
    if c["name"] not in _TOL:
        _TOL[c["name"]] = sl.tolerance(**inputs(c))
    return _TOL[c["name"]]


def differences(c, got, with_row=True):
    """depth_measure_cases.differences against this file's expectation: the same scheme, bounds from the planted ulps"""
    want, bound = expected(c)
    bad, ratio = {}, {}
    for k in ("outcome", "n_failed", "status"):
        if got[k] != want[k]:
            bad[k] = (got[k], want[k], 0)
    gn, wn = dr._numbers(got), dr._numbers(want)
    if not with_row:
        gn, wn = ({k: v for k, v in d.items() if not k.startswith("row.")} for d in (gn, wn))
    for k in sorted(set(gn) | set(wn)):
        if k not in gn or k not in wn:
            bad[k] = (gn.get(k), wn.get(k), None)
        elif wn[k] != wn[k] or gn[k] != gn[k]:
            if not (wn[k] != wn[k] and gn[k] != gn[k]):
                bad[k] = (gn[k], wn[k], None)
        else:
            d = abs(gn[k] - wn[k])
            ratio[k] = d / bound[k] if bound[k] > 0 else (0.0 if d == 0 else math.inf)
            if d > bound[k]:
                bad[k] = (gn[k], wn[k], bound[k])
    for k in ("n_failed", "fixed", "trash") if with_row else ():
        if got["row"].get(k) != want["row"].get(k):
            bad["row." + k] = (got["row"].get(k), want["row"].get(k), 0)
    return bad, ratio


def check(c):
    """asserts, on the CPU, that the restatement takes the case where its name says"""
    base = sl.restate(**inputs(c))
    want = c["want"]
    if "status" in want:
        assert base["status"] == want["status"], (c["name"], base["status"], want["status"])
    if "outcome" in want:
        assert base["outcome"] == want["outcome"], (c["name"], base["outcome"], want["outcome"])
    if want.get("updated"):
        assert base["outcome"] in (UPDATED, CONVERGED) and base["status"] == sr.OK, (c["name"], base["outcome"], base["status"])
    if "position" in want:
        assert base["position"] == tuple(want["position"]), (c["name"], base["position"])
    if base["status"] == sr.OK:
        assert len(sl.spread_outcomes(**inputs(c))) == 1, (c["name"], "the outcome depends on the last bits of exp")
    return base
