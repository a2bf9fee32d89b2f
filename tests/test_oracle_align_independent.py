"""The ORACLE's sparse image alignment (ImageAlign::ComputePose, Optimize, ComputeResiduals, PrecomputePatches: oracle/ref_align.h)
against a float64 numpy restatement written from the reference's text (tests/align_restatement.py), on the named cases of
tests/align_cases.py: reference keyframes rolled 30 and 90 degrees, tilted 25 and zoomed 0.6 and 1.9 away from the world frame, a
tilted scene plane (depths 2.0 to 4.0), a current view rolled 8 degrees against its reference, features that leave the current
image at a level's first evaluation and later, a start 0.2 m and 0.1 rad off, levels (0,4), (4,4), (0,0), iteration limits 1 and 2,
both branches of a fast call, a start that measures nothing, a band of features no coarse level sees (n_meas == 0 on a non-empty
job, then the sticky stop), a NaN system, flat images, depths scaled by 0.02, 50, -1 and 0, points behind and exactly on the
current camera plane, and 752- and 330-pixel frames whose level widths are no multiples of 4.  Until now the tests of the alignment
showed only that csrc/sdvl_image_align.hip equals the oracle, on inputs that start at the identity on the plane z = 2 of the world.

Measured 2026-10-18 over the 31 committed cases and the 6 variants of 385 to 450 features (the figures are printed by the tests, run
with -s):
* Oracle against restatement: n_meas, its at every level, stop, the number of evaluations and the fast / stop branch are equal on all
  37 runs.  The 4x4 poses of the multi-iteration runs differ by 1.7e-8 to 9.5e-8 (levels-0-0; its2 9.4e-8, step-roll8 8.1e-8; by 0 on the four
  cases whose pose must not move): the
  restatement has no float32, the reference rounds every level position to float (image_align.cc:165-166, 225-226: 3e-5 of a pixel
  at x = 300, 6e-5 from 512 on) and every intensity (1.5e-5 of a grey level).  Rounding the interpolated intensities alone moves
  the restatement's pose by 3e-10 to 2e-9; the positions account for the rest, through the direction in which a sideways
  translation and a turn about the vertical axis nearly cancel on a plane.  ALIGN_BOUND is 100 times the largest, 9.5e-6, and is
  asserted to stay at or below POSE_TOL / 10 = 1e-5.  It does so by a hair, and by the choice of frame: the level-0-only case on
  640x480 (x up to 592) measured 1.6e-7, which times 100 is above 1e-5, so levels-0-0 runs on the 330x250 frame, where the float
  spacing of the positions is half as wide.  What this says about the device tolerance: two correct implementations that round the
  positions differently are up to 1.6e-7 apart, three orders below POSE_TOL; the kernel rounds them as the oracle does.
* One-evaluation runs: 4.6e-9 to 7.2e-8, and 2.5e-7 on zero-z, whose single step is 0.22 long.  ONE_EVAL_BOUND is 100 times that, 2.5e-5.
  w330-one (a frame aligned with itself from the identity) gives 2.8e-17 and chi2 exactly 0 on the oracle.
* Branches taken, summed over the 37 runs: rollback 72, step-size stop 4, out of iterations 14, measured set changed at a level's
  first evaluation 42 and at a later one 48, fast early-out 2, stop by n_meas 7, stop by NaN 3.
* Admission screen (n_meas, its, stop and branch unchanged when the start pose, and again every depth, moves one ulp up and one
  down): every case passed on its first seed, none was discarded.  zero-z rests on two sums that are exactly 0, which one ulp on the
  start or on its two constructed depths undoes by design: there the screen moves the other 98 depths only.
* Planted faults, cases of 31 that separate each from the oracle (another n_meas or stop, its more than 1 apart, or a pose more
  than 10 x POSE_TOL away): update_side 6 (step-roll8, leaving-later, far-start, fast-exact by its; behind-tz-4 by 3.7e-2, zero-z),
  jacobian_at_current_point 7, focal_not_scaled 25, depth_is_z 22, h_keeps_departed 9, border_gt 9, rollback_keeps_current 6,
  chi2_compared_at_it0 15, stop_not_sticky 1 (band-no-level4), fast_ignored 1 (fast-early), invalid_counted 30.
* The legacy inputs (test_gpu_parity.py::test_image_align_pose_within_tolerance: identity start, plane z = 2, reference = world; the
  restatement agrees with the oracle on all four jobs, 2.5e-8 to 4.1e-7) do NOT separate h_keeps_departed, border_gt,
  stop_not_sticky and fast_ignored: no feature of theirs leaves the image, stop_ is never set, and their fast job (200, 40) does not
  take the early-out.  update_side is separated only by the job of 7 features (6 measured), by its 2 against 4 at level 2 and a pose
  3.8e-3 away on a system that 6 features barely determine; the three larger jobs do not separate it.
* No kernel or oracle fault was found: the oracle does not depart from image_align.cc on any case.
"""
import numpy as np
import pytest

from align_cases import BIG_CASES, CASES, MULTI_CASES, ONE_EVAL_CASES, case, frames, oracle_answer
from align_restatement import BRANCHES, FAULTS, restate
from oraclelib import TUM_CAM, trajectory_pose
from pose_restatement import SE3_IDENTITY, se3_matrix

POSE_TOL = 1e-4                 # the device tolerance of the alignment's pose (tests/test_gpu_parity.py, BASELINE.json)
ALIGN_BOUND = 9.5e-6            # 100 x the largest oracle-to-restatement distance over the multi-iteration cases (9.5e-8), see above
assert ALIGN_BOUND <= POSE_TOL / 10
ONE_EVAL_BOUND = 2.5e-5         # 100 x the largest over the one-evaluation cases (2.5e-7, zero-z: one step of 0.22), see above
# the case that is asserted to separate each planted fault from the oracle (any one would do; the docstring lists how many do)
WITNESS = {
    "update_side": "behind-tz-4", "jacobian_at_current_point": "leaving", "focal_not_scaled": "ref-roll30", "depth_is_z": "leaving",
    "h_keeps_departed": "ref-roll30", "border_gt": "leaving", "rollback_keeps_current": "tilted-plane",
    "chi2_compared_at_it0": "ref-roll90", "stop_not_sticky": "band-no-level4", "fast_ignored": "fast-early", "invalid_counted": "ref-roll30",
}
LEGACY = [(200, 3, False), (1000, 5, False), (200, 40, True), (7, 2, False)]     # test_image_align_pose_within_tolerance
EVERY = [(k, False) for k in CASES] + [(k, True) for k in BIG_CASES]

_restated, _wanted, _pyr = {}, {}, {}


def wanted(orc, synth, name, big=False):
    if (name, big) not in _wanted:
        _wanted[(name, big)] = oracle_answer(orc, synth, case(name), big=big)
    return _wanted[(name, big)]


def pyramids(orc, synth, c):
    out = []
    for img in frames(synth, c):
        if id(img) not in _pyr:
            _pyr[id(img)] = (img, orc.pyramid(img, 5))        # (the frames are uint8 inputs of both sides: Frame::GetPyramid)
        out.append(_pyr[id(img)][1])
    return out


def restated(orc, synth, name, big=False, fault=None):
    if (name, big, fault) not in _restated:
        c = case(name)
        f = c["feats_big"] if big else c["feats"]
        p1, p2 = pyramids(orc, synth, c)
        _restated[(name, big, fault)] = restate(p1, p2, c["cam"], f["px"], f["bearing"], f["depth"], f["valid"], c["start"], fast=c["fast"],
                                                fault=fault, **c["limits"])
    return _restated[(name, big, fault)]


def pose_distance(a, b):
    return float(np.abs(se3_matrix(a["T"]) - se3_matrix(b["T"])).max())


def same_decisions(a, b):
    """n_meas, its, stop and the fast / stop branch (error is 1e10 on both sides or on neither)"""
    return (a["n"] == b["n"] and np.array_equal(a["its"], b["its"]) and a["stop"] == b["stop"]
            and (a["error"] == 1e10) == (b["error"] == 1e10))


def separated(want, got):
    """the issue's measure: another n_meas or stop, its more than 1 apart at some level, or a pose more than 10 x POSE_TOL away"""
    return (want["n"] != got["n"] or want["stop"] != got["stop"] or int(np.abs(want["its"] - got["its"]).max()) > 1
            or pose_distance(want, got) > 10 * POSE_TOL)


@pytest.mark.parametrize("name,big", EVERY)
def test_every_case_is_stable_on_the_oracle(orc, synth, name, big):
    """the admission screen of tests/align_cases.py, run on every committed case: the start pose, and again every depth, moved one
    ulp up and one ulp down leaves the oracle's n_meas, its, stop and branch as they are.  zero-z is built on two exact zeros: there
    the screen moves the depths of the features that are not the two constructed ones, and not the start."""
    c, w = case(name), wanted(orc, synth, name, big)
    f = c["feats_big"] if big else c["feats"]
    for sign in (1.0, -1.0):
        moved_depth = np.nextafter(f["depth"], sign * np.inf)
        moves = [("depth", dict(depth=moved_depth))]
        if c["extra"] == "zero-z":
            moved_depth[1:3] = f["depth"][1:3]
        else:
            moves.append(("start pose", dict(start=np.nextafter(c["start"], sign * np.inf))))
        for what, kw in moves:
            v = oracle_answer(orc, synth, c, big=big, **kw)
            assert same_decisions(w, v), (name, what, sign, w["n"], v["n"], w["its"], v["its"], w["stop"], v["stop"])


@pytest.mark.parametrize("name,big", EVERY)
def test_oracle_equals_the_restatement(orc, synth, name, big):
    c, w, r = case(name), wanted(orc, synth, name, big), restated(orc, synth, name, big)
    d = pose_distance(w, r)
    print("%s%s: n %d, its %s, stop %d, evals %d, error %.2e, pose %.1e from the restatement's; %s"
          % (name, "+" if big else "", w["n"], w["its"][:5].tolist(), w["stop"], w["evals"], w["error"], d, {k: v for k, v in r["trace"].items() if v}))
    assert w["n"] == r["n"] and w["stop"] == r["stop"], (w["n"], r["n"], w["stop"], r["stop"])
    assert (w["error"] == 1e10) == (r["error"] == 1e10)
    assert np.array_equal(w["its"], r["its"]), (w["its"], r["its"])
    assert w["evals"] == r["evals"]
    assert d <= (ONE_EVAL_BOUND if c["one_eval"] else ALIGN_BOUND), d
    # the float running sum of :192 over 16 n terms; w330-one aligns a frame with itself: 0 exactly in float, in float64 the square of
    # the reprojection's own rounding (1e-13 px times the gradient)
    assert abs(w["chi2"] - r["chi2"]) <= 16 * w["n"] * 2.0 ** -24 * abs(w["chi2"]) + 1e-20


def test_the_bounds_are_what_was_measured(orc, synth):
    """ALIGN_BOUND and ONE_EVAL_BOUND are 100 x the largest distance of their class, to two digits, not a looser number"""
    multi = max(pose_distance(wanted(orc, synth, n, b), restated(orc, synth, n, b)) for n, b in EVERY if n in MULTI_CASES)
    one = max(pose_distance(wanted(orc, synth, n, b), restated(orc, synth, n, b)) for n, b in EVERY if n in ONE_EVAL_CASES)
    print("largest oracle-to-restatement distance: multi-iteration %.2e, one evaluation %.2e" % (multi, one))
    assert 50 * multi <= ALIGN_BOUND <= 200 * multi and 50 * one <= ONE_EVAL_BOUND <= 200 * one


def test_the_cases_reach_what_they_are_there_for(orc, synth):
    """every branch of the trace is taken somewhere, and each special case ends where the issue that asked for it says"""
    total = dict.fromkeys(BRANCHES, 0)
    for name, big in EVERY:
        for k in BRANCHES:
            total[k] += restated(orc, synth, name, big)["trace"][k]
    print("branches over %d runs: %s" % (len(EVERY), total))
    for k in BRANCHES:
        assert total[k] > 0, k
    W = {n: wanted(orc, synth, n) for n in CASES}
    for n in ("ref-roll30", "ref-roll90", "ref-tilt25", "ref-zoom0.6", "ref-zoom1.9-roll20", "tilted-plane", "far-start", "leaving"):
        c = case(n)
        d = float(np.abs(se3_matrix(W[n]["T"]) - se3_matrix(c["T_rel"])).max())
        assert d < 5e-3 and d < 0.5 * np.abs(se3_matrix(c["start"]) - se3_matrix(c["T_rel"])).max(), (n, d)    # it aligns the frames
    assert case("tilted-plane")["feats"]["depth"].max() > 3.9 and case("ref-zoom1.9-roll20")["feats"]["depth"].max() < 1.3
    nv = int(case("leaving")["feats"]["valid"].sum())
    assert W["leaving"]["n"] <= nv - 20 and restated(orc, synth, "leaving")["trace"]["set_changed_later"] > 0
    assert restated(orc, synth, "leaving-at-it0")["trace"]["set_changed_it0"] == 3
    t = restated(orc, synth, "leaving-later")["trace"]
    assert t["set_changed_it0"] == 0 and t["set_changed_later"] > 0
    assert W["far-start"]["its"][4] >= 10
    assert all(W["levels-0-4"]["its"][:5] > 0) and W["levels-4-4"]["its"][4] > 0 and W["levels-0-0"]["its"][0] > 0
    assert list(W["its1"]["its"][:5]) == [0, 0, 1, 1, 1] and list(W["its2"]["its"][:5]) == [0, 0, 2, 2, 2]
    # fast: the early-out after the coarsest level (the same start without `fast` is its1, which goes on), and no early-out
    assert list(W["fast-early"]["its"][:5]) == [0, 0, 0, 0, 1] and W["fast-early"]["error"] == 1e10 and W["fast-early"]["evals"] == 1
    assert np.array_equal(case("fast-early")["start"], case("its1")["start"]) and W["its1"]["error"] < 1e9
    assert all(W["fast-exact"]["its"][2:5] > 0) and W["fast-exact"]["error"] < 0.01
    for n in ("nothing-measured", "band-no-level4", "nan-depth0"):                  # stop: by n_meas (twice) and by NaN
        w = W[n]
        assert np.array_equal(w["T"], case(n)["start"]) and w["stop"] == 1 and not w["its"].any() and w["error"] == 1e10 and w["chi2"] == 1e10
        assert w["evals"] == 3
    assert W["nothing-measured"]["n"] == 0 and W["band-no-level4"]["n"] > 60 and W["nan-depth0"]["n"] > 40
    assert restated(orc, synth, "nan-depth0")["trace"]["stop_nan"] == 3 and restated(orc, synth, "band-no-level4")["trace"]["stop_n_meas"] == 1
    w = W["flat-reference"]
    assert np.array_equal(w["T"], case("flat-reference")["start"]) and w["its"][:5].tolist() == [0, 0, 1, 1, 1] and w["error"] == 0.0 and w["stop"] == 0
    # depth edges: scaled depths measured in part; behind the camera the mirrored projections land inside; the two exact zeros
    for n in ("depth-mix-l2", "depth-mix-l4"):
        assert 0.6 * case(n)["n"] < W[n]["n"] < int(case(n)["feats"]["valid"].sum()), (n, W[n]["n"])
    assert W["behind-tz-4"]["n"] > 150
    c = case("zero-z")
    P = c["feats"]["bearing"] * c["feats"]["depth"][:, None] + c["start"][4:]
    assert P[1, 2] == 0.0 and P[1, 0] == 0.0 and P[1, 1] == 0.0 and P[2, 2] == 0.0 and P[2, 0] != 0.0
    assert (np.delete(P[:, 2], [1, 2]) > 1.0).all() and 20 < W["zero-z"]["n"] < 98
    for n, widths in (("w752", (188, 94, 47)), ("w330", (330, 165, 82, 41))):
        c = case(n)
        assert tuple(c["size"][0] >> l for l in range(c["limits"]["min_level"], c["limits"]["max_level"] + 1)) == widths
        assert sum(1 for x in widths if x % 4) >= 2


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_case_separates_each_planted_fault(orc, synth, fault):
    """the restatement with ONE error planted (align_restatement.FAULTS) no longer agrees with the oracle on its witness case:
    another n_meas or stop, its more than 1 apart, or a pose more than 10 x POSE_TOL away.  Without the error the same case agrees
    (test above)."""
    hits = [n for n in CASES if separated(wanted(orc, synth, n), restated(orc, synth, n, fault=fault))]
    name = WITNESS[fault]
    w, r = wanted(orc, synth, name), restated(orc, synth, name, fault=fault)
    print("%s: separated by %d cases %s; on %s: n %d / %d, its %s / %s, stop %d / %d, pose %.1e apart"
          % (fault, len(hits), hits, name, w["n"], r["n"], w["its"][:5].tolist(), r["its"][:5].tolist(), w["stop"], r["stop"], pose_distance(w, r)))
    assert separated(w, r), (fault, name)


def legacy_inputs(orc, synth, n_feat, k):
    """the inputs of test_gpu_parity.py::test_image_align_pose_within_tolerance: frames 0 and k of the trajectory, align_inputs' features
    of frame 0 on the plane z = 2 (camera 0 = world), start at the identity"""
    img0, imgk = (synth.render(trajectory_pose(orc, j), TUM_CAM, 640, 480, seed=20260001, frame_id=j) for j in (0, k))
    rng = np.random.default_rng(20260200)
    px = np.stack([rng.uniform(48, 640 - 48, n_feat), rng.uniform(48, 480 - 48, n_feat)], 1)
    ray = np.stack([(px[:, 0] - TUM_CAM[2]) / TUM_CAM[0], (px[:, 1] - TUM_CAM[3]) / TUM_CAM[1], np.ones(n_feat)], 1)
    bearing = ray / np.linalg.norm(ray, axis=1, keepdims=True)
    depth = 2.0 / bearing[:, 2]
    valid = np.ones(n_feat, np.uint8)
    valid[::17] = 0
    return img0, imgk, px, bearing, depth, valid


def test_which_faults_the_legacy_inputs_separate(orc, synth):
    """The same faults over the inputs the alignment was tested with so far (identity start, reference = world, plane z = 2).  A job
    counts only where the restatement WITHOUT a fault agrees with the oracle.  Recorded in the module docstring; asserted: the sticky stop, the
    ignored fast flag and the departed features' H are among the faults those inputs miss (they never set stop_, their fast job does
    not take the early-out, and no feature of theirs leaves the image)."""
    jobs = []
    for n_feat, k, fast in LEGACY:
        img0, imgk, px, bearing, depth, valid = legacy_inputs(orc, synth, n_feat, k)
        w = orc.image_align(img0, imgk, TUM_CAM, px, bearing, depth, valid, SE3_IDENTITY, fast=fast)
        args = (orc.pyramid(img0, 5), orc.pyramid(imgk, 5), TUM_CAM, px, bearing, depth, valid, SE3_IDENTITY)
        r = restate(*args, fast=fast)
        agrees = same_decisions(w, r) and pose_distance(w, r) <= ALIGN_BOUND
        print("legacy job (%d, %d, %s): n %d, its %s, error %.1e, restatement %s (%.1e)"
              % (n_feat, k, fast, w["n"], w["its"][:5].tolist(), w["error"], "agrees" if agrees else "does NOT agree", pose_distance(w, r)))
        if agrees:
            jobs.append((n_feat, args, fast, w))
    assert len(jobs) >= 3
    missed = []
    for fault in FAULTS:
        hit = None
        for n_feat, args, fast, w in jobs:
            r = restate(*args, fast=fast, fault=fault)
            if separated(w, r):
                hit = (n_feat, w["n"], r["n"], w["its"][2:5].tolist(), r["its"][2:5].tolist(), pose_distance(w, r))
                break
        print("%s: %s" % (fault, "separated by the job of %d features (n %d / %d, its %s / %s, pose %.1e apart)" % hit if hit
                          else "NOT separated by any legacy job"))
        if hit is None:
            missed.append(fault)
    print("faults the legacy inputs miss: %s" % missed)
    assert {"stop_not_sticky", "fast_ignored", "h_keeps_departed"} <= set(missed), missed
