"""K7 (`search_prepare` / `search_points`, and phase 0 inside `track_project_kernel`) against the oracle under warps far from the
identity: the current view rolled 30 and 90 degrees, tilted 25 degrees with a sideways baseline, zoomed 1.9x with a 20 degree roll,
zoomed out to 0.6x (oraclelib.WARP_VIEWS; the oracle's own reading of matcher.cc:293-357 on exactly these requests is pinned by
tests/test_oracle_warp_independent.py).  Every decision equal, offsets bit-identical (the class of K7)."""
import importlib
import math

import numpy as np
import pytest

from oraclelib import TUM_CAM, WARP_CAM, WARP_VIEWS, fill_search_reqs, quat_to_R, trajectory_pose, warp_border_case, warp_view_case
from warp_restatement import restate_border_case

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4
CASES = [(v, f) for v in WARP_VIEWS for f in (True, False)]
IDS = ["%s-%s" % (v, "fixed" if f else "epipolar") for v, f in CASES]


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trk():
    importlib.import_module("slam-sdvl_amd")
    return importlib.import_module("slam-sdvl_amd.tracker")


def make_reqs(sdvl, case, f_ref, f_cur, fixed, meta=None):
    return fill_search_reqs(sdvl, case["meta"] if meta is None else meta, f_ref, f_cur, case["T_ref"], case["T_cur"], fixed)


def mismatches(res, want, ccur):
    """requests whose result differs from the oracle's in any decision or, where found, in any bit of px"""
    bad = []
    for i, (r, w) in enumerate(zip(res, want)):
        ok = r.found == w["found"] and r.stage == w["stage"] and r.level == w["level"]
        ok = ok and r.slevel == (w["slevel"] if w["stage"] >= 1 else -1)
        ok = ok and (r.best_corner >= 0) == (w["best_corner"] >= 0)
        if ok and w["best_corner"] >= 0:
            ok = tuple(ccur[r.best_corner]) == tuple(ccur[w["best_corner"]])
        if ok and w["stage"] >= 2:     # the chosen corner (LK did not converge) or the refined position (found), bit for bit
            ok = np.array_equal(np.array(r.px[:]), w["px"])
        if not ok:
            bad.append((i, (r.found, r.stage, r.level, r.slevel, r.best_corner, tuple(r.px)),
                        (w["found"], w["stage"], w["level"], w["slevel"], w["best_corner"], tuple(w["px"]))))
    return bad


def check_inputs(case, view):
    """conditions on the INPUTS, judged on the oracle alone"""
    want = case["want"]
    n_found = sum(w["found"] for w in want)
    assert len(want) == 120 and n_found >= case["found_floor"], (n_found, case["found_floor"])
    levels = {w["slevel"] for w in want if w["stage"] >= 1}
    assert levels == ({1, 2} if view.startswith("zoom1.9") else {0, 1} if view.startswith("zoom0.6") else {0, 1, 2}), levels


def isolation_layer(ctx, f_cur, res, want, ccur):
    """AlignPatch alone: the ORACLE's patches and the oracle's winning corner into sdvl_align_patches -> requests whose offsets are
    not, bit for bit, the oracle's and the ones search_points returned"""
    idx = [i for i, w in enumerate(want) if w["found"]]
    if not idx:
        return []
    border = np.stack([want[i]["border"] for i in idx])
    patch = np.stack([want[i]["border"].reshape(10, 10)[1:9, 1:9].reshape(-1) for i in idx])
    sl = np.array([want[i]["slevel"] for i in idx], np.int32)
    best = ccur[[want[i]["best_corner"] for i in idx]]
    uv0 = best[:, :2] * (1 << best[:, 2:3]).astype(np.float64) / (1 << sl)[:, None]     # px / (1 << slevel), matcher.cc:113
    uv, conv, _ = ctx.align_patches([f_cur] * len(idx), sl, border, patch, uv0)
    bad = []
    for k, i in enumerate(idx):
        px = uv[k] * (1 << int(sl[k]))
        if not (conv[k] == 1 and np.array_equal(px, want[i]["px"]) and np.array_equal(px, np.array(res[i].px[:]))):
            bad.append((i, int(conv[k]), tuple(px), tuple(want[i]["px"]), tuple(res[i].px)))
    return bad


def verdict(whole, iso):
    if not whole and not iso:
        return ""
    if whole and not iso:
        where = "the LK alone reproduces the oracle from the oracle's patches: the fault is in CreatePatch (phase 0's warp included) or in the match"
    elif whole:
        where = "the LK alone fails on the oracle's own patches too: the fault is in the LK (align_patch_wave)"
    else:
        where = "search_points agrees with the oracle but sdvl_align_patches does not: the fault is in the stand-alone LK entry"
    return "%d whole-kernel mismatches (request, device, oracle) %s; %d isolation-layer mismatches %s: %s" % (len(whole), whole[:4], len(iso), iso[:4], where)


@pytest.mark.parametrize("view,fixed", CASES, ids=IDS)
def test_search_points_equals_oracle_under_the_warp(ctx, sdvl, orc, synth, view, fixed):
    """ORB matching with the frame's descriptors in HBM and computed on demand; then AlignPatch in isolation"""
    case = warp_view_case(orc, synth, view, fixed)
    check_inputs(case, view)
    cam = sdvl.Camera(640, 480, *WARP_CAM)
    for describe in (True, False):
        f_ref, f_cur = ctx.frame(case["img_ref"]), ctx.frame(case["img_cur"])
        try:
            f_cur.set_corners(case["ccur"])
            if describe:
                ctx.orb_describe([f_cur], want=False)
            res = ctx.search_points(make_reqs(sdvl, case, f_ref, f_cur, fixed), cam, sdvl.default_search_params())
            whole = mismatches(res, case["want"], case["ccur"])
            iso = isolation_layer(ctx, f_cur, res, case["want"], case["ccur"])
        finally:
            f_ref.close(); f_cur.close()
        assert not whole and not iso, "descriptors %s: %s" % ("in HBM" if describe else "on demand", verdict(whole, iso))


@pytest.mark.parametrize("view,fixed", CASES, ids=IDS)
def test_search_points_zmssd_equals_oracle_under_the_warp(ctx, sdvl, orc, synth, view, fixed):
    """use_orb = 0: the warped patch's own sums pick the corner, so a wrong patch pixel shows where the ORB winner would not change"""
    case = warp_view_case(orc, synth, view, fixed, use_orb=False)
    check_inputs(case, view)
    f_ref, f_cur = ctx.frame(case["img_ref"]), ctx.frame(case["img_cur"])
    try:
        f_cur.set_corners(case["ccur"])
        res = ctx.search_points(make_reqs(sdvl, case, f_ref, f_cur, fixed), sdvl.Camera(640, 480, *WARP_CAM), sdvl.default_search_params(use_orb=False))
        whole = mismatches(res, case["want"], case["ccur"])
        iso = isolation_layer(ctx, f_cur, res, case["want"], case["ccur"])
    finally:
        f_ref.close(); f_cur.close()
    assert not whole and not iso, verdict(whole, iso)


BORDER_FLOOR = {"roll30": (6, 12), "zoom0.6": (10, 6)}     # half of what the oracle gives, as for the found floors of the views


@pytest.mark.parametrize("view", ["roll30", "zoom0.6"])
def test_patches_that_leave_the_reference_image_equal_the_oracle(ctx, sdvl, orc, synth, view):
    """CreatePatch's out-of-image rule under a warp: points 6 to 9 pixels inside each border of the reference image
    (oraclelib.warp_border_case), whose rolled or spread sample grids cross it, with ZMSSD matching: a zeroed sample in the inner
    8x8 enters the sums that pick the corner, one in the outer ring enters the LK.  Stage, winning corner and px as the oracle's,
    bit for bit.  On the inputs (oracle and restatement alone): of 180 requests 37 / 34 (roll 30 / zoom 0.6) have samples outside,
    12 / 21 of those still pick a corner and refine it (all their outside samples in the ring), 25 / 13 stop at the match."""
    case = warp_border_case(orc, synth, view)
    want = case["want"]
    restated = restate_border_case(orc, case)
    zeroed = sum(int(r["outside"].sum()) for r in restated)
    assert zeroed >= 40 and 100 * len(restated) - zeroed >= 10 * zeroed, zeroed      # the inputs do cross the border, and only just
    crossing = [bool(r["outside"].any()) for r in restated]
    n_lk = sum(c and w["stage"] >= 2 for c, w in zip(crossing, want))
    n_match = sum(c and w["stage"] == 1 for c, w in zip(crossing, want))
    print("%s: %d requests cross the border, %d of them reach the LK, %d stop at the match" % (view, sum(crossing), n_lk, n_match))
    assert n_lk >= BORDER_FLOOR[view][0] and n_match >= BORDER_FLOOR[view][1], (n_lk, n_match)
    f_ref, f_cur = ctx.frame(case["img_ref"]), ctx.frame(case["img_cur"])
    try:
        f_cur.set_corners(case["ccur"])
        res = ctx.search_points(make_reqs(sdvl, case, f_ref, f_cur, True), sdvl.Camera(640, 480, *WARP_CAM), sdvl.default_search_params(use_orb=False))
        whole = mismatches(res, want, case["ccur"])
        iso = isolation_layer(ctx, f_cur, res, want, case["ccur"])
    finally:
        f_ref.close(); f_cur.close()
    assert not whole and not iso, verdict(whole, iso)


def region_class(case, m, slevel):
    """what the corner bins can do for an epipolar request, from the spread of the projected depth interval (matcher.cc:66-76) alone:
    1 the box around the segment misses the 20 x 15 grid of 32-pixel cells, 2 it covers at most four cell rows and 320 cells,
    0 it is larger.  -> (class, length of the segment in pixels)"""
    assert np.array_equal(case["T_ref"], [1, 0, 0, 0, 0, 0, 0])
    R, t = quat_to_R(case["T_cur"][:4]), case["T_cur"][4:]
    ends = []
    for z in (1.0 / (m["idepth"] + 2.0 * m["istd"]), 1.0 / max(m["idepth"] - 2.0 * m["istd"], 1e-8)):
        p = R @ (z * m["bearing"]) + t
        ends.append([WARP_CAM[2] + WARP_CAM[0] * p[0] / p[2], WARP_CAM[3] + WARP_CAM[1] * p[1] / p[2]])
    a, b = np.array(ends)
    rng = 6.0 * 1.2 ** slevel
    lo, hi = np.minimum(a, b) - rng, np.maximum(a, b) + rng
    cx0, cx1 = max(0, math.floor(lo[0]) >> 5), min(19, math.floor(hi[0]) >> 5)
    cy0, cy1 = max(0, math.floor(lo[1]) >> 5), min(14, math.floor(hi[1]) >> 5)
    seg = float(np.linalg.norm(a - b))
    if cx1 < cx0 or cy1 < cy0:
        return 1, seg
    return (2 if cy1 - cy0 < 4 and (cx1 - cx0 + 1) * (cy1 - cy0 + 1) <= 320 else 0), seg


@pytest.mark.parametrize("view", list(WARP_VIEWS) + ["zoom1.9-roll20-wide"])
def test_epipolar_search_on_a_binned_frame_under_the_warp(ctx, sdvl, orc, synth, view):
    """the same epipolar requests against the current frame with corner bins (sdvl_detect_corners, which returns the oracle's list)
    and without (set_corners): same results, equal to the oracle's.  What the bins are asked for differs per view, computed here
    from the segments.  region_class models the size of the region alone: a segment that is too short to have a direction (zero
    length, or a normal that is not finite) is searched without a prepared region whatever its size, so the pure rolls, which have no
    baseline (segments of < 1e-9 px, a direction made of rounding), may be searched either way: device and oracle must still agree.
    The tilt and the zooms project the +-20 % depth interval onto 2 to 260 px; with these intervals no region exceeds four cell
    rows; the -wide case (idepth_std 40 % of idepth: the far end at five times the depth) adds the regions that do.
    Measured, requests by class (0, 1, 2) and what the oracle finds in each: roll 30 (0, 7, 113) finds (0, 0, 54); roll 90
    (0, 17, 103) finds (0, 1, 39); tilt 25 (0, 3, 117) finds (0, 0, 24); zoom 1.9 + roll 20 (0, 63, 57) finds (0, 0, 9); zoom 0.6
    (0, 0, 120) finds (0, 0, 6); zoom 1.9 + roll 20 wide (56, 10, 54) finds (6, 0, 3), longest segment 2080 px.  The floors on the
    wide case are half of its figures."""
    base = view.replace("-wide", "")
    case = warp_view_case(orc, synth, base, False)
    meta, want = case["meta"], case["want"]
    if view.endswith("-wide"):
        meta = [dict(m, istd=0.4 * m["idepth"]) for m in meta]
        want = [orc.search_point(case["img_ref"], case["img_cur"], WARP_CAM, case["T_ref"], case["T_cur"], m["px"], m["bearing"], m["level"],
                                 m["desc"], m["idepth"], m["istd"], False, case["ccur"], m["px0"]) for m in meta]
    else:
        check_inputs(case, view)
    cls = [region_class(case, m, w["slevel"]) for m, w in zip(meta, want)]
    kinds = {c for c, _ in cls}
    longest = max(s for _, s in cls)
    print("%s: regions by class %s, longest segment %.3g px, oracle finds %d" % (view, np.bincount([c for c, _ in cls], minlength=3), longest, sum(w["found"] for w in want)))
    if base.startswith("roll"):
        assert longest < 1e-9 and kinds == {1, 2}
    elif view.endswith("-wide"):
        large = [w["found"] for (c, _), w in zip(cls, want) if c == 0]
        assert {0, 2} <= kinds and len(large) >= 28 and sum(large) >= 3 and sum(w["found"] for w in want) >= 4
    elif base == "zoom0.6":
        assert kinds == {2} and longest > 20
    else:
        assert kinds == {1, 2} and longest > 100
    cam = sdvl.Camera(640, 480, *WARP_CAM)
    f_ref, f_cur, f_bin = ctx.frame(case["img_ref"]), ctx.frame(case["img_cur"]), ctx.frame(case["img_cur"])
    try:
        f_cur.set_corners(case["ccur"])
        detected = ctx.detect_corners([f_bin], sdvl.default_detect_params(), 1000)[0]
        assert np.array_equal(detected, case["ccur"])
        plain = ctx.search_points(make_reqs(sdvl, case, f_ref, f_cur, False, meta), cam, sdvl.default_search_params())
        binned = ctx.search_points(make_reqs(sdvl, case, f_ref, f_bin, False, meta), cam, sdvl.default_search_params())
        bad_plain, bad_binned = mismatches(plain, want, case["ccur"]), mismatches(binned, want, case["ccur"])
        differ = [i for i, (a, b) in enumerate(zip(plain, binned))
                  if (a.found, a.stage, a.level, a.slevel, a.best_corner, tuple(a.px)) != (b.found, b.stage, b.level, b.slevel, b.best_corner, tuple(b.px))]
    finally:
        f_ref.close(); f_cur.close(); f_bin.close()
    assert not differ and not bad_plain and not bad_binned, (differ[:8], bad_plain[:4], bad_binned[:4])


ROLL_STEP_DEG = 4.0     # the oracle tracker stays TRACKING at this step (state 2, quality 0; measured on the CPU: 55 to 200 matches a frame, asserted >= 50)


def test_closed_loop_through_a_roll_of_forty_degrees(trk, orc, synth):
    """track_project_kernel's copy of phase 0 under a real rotation: six frames of the usual trajectory, then the camera rolls
    4 degrees a frame about its optical axis for ten frames, 40 degrees against the first keyframe.  Every per-frame decision as the
    oracle tracker's, poses within 1e-4."""
    trk.configure()
    dev = trk.HostDevice(0)
    batch = trk.TrackerBatch(dev, 1, 640, 480, TUM_CAM)
    ref = orc.tracker(640, 480, TUM_CAM)
    T5 = trajectory_pose(orc, 5)
    try:
        for k in range(16):
            T = trajectory_pose(orc, k) if k < 6 else orc.se3_mul(orc.se3_exp([0, 0, 0, 0, 0, math.radians(ROLL_STEP_DEG * (k - 5))]), T5)
            img = synth.render(T, TUM_CAM, 640, 480, frame_id=k)
            g = batch.step_host([img])[0]
            w = ref.handle_frame(img)
            assert g.host_path == 0, (k, g.host_path)      # on the device-resident tables: track_project_kernel did this frame's phase 0
            assert (g.state, g.quality, g.keyframe, g.n_corners) == (w.state, w.quality, w.keyframe, w.n_corners), k
            assert (g.matches, g.attempts, g.inliers, g.outliers) == (w.matches, w.attempts, w.inliers, w.outliers), k
            assert g.align_meas == w.align_meas and g.relocalized == w.relocalized == 0, k
            assert np.abs(np.array(g.pose[:]) - np.array(w.pose[:])).max() <= POSE_TOL, k
            if k > 0:
                assert w.state == 2 and w.quality == 0 and w.matches >= 50, (k, w.state, w.quality, w.matches)   # the ORACLE keeps tracking
    finally:
        batch.close(); ref.close(); dev.close()
