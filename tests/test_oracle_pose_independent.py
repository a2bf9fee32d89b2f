"""The ORACLE's pose stage (SelectInliers, ConvergePose, OptimizePose, RescueOutliers: oracle/ref_tracker.h) against a float64 numpy
restatement written from the reference's text (tests/pose_restatement.py), on the named cases of tests/pose_cases.py: start poses
rolled 30, 90 and exactly 180 degrees and turned 100 degrees about an oblique axis with metres of translation, levels 0 to 4, depths
down to 0.15, points behind the start camera, repeated observations, 1 to 1024 matches, outlier shares 0 to 0.65, and every limit
away from its default.  Until now the GPU tests of the stage showed only that csrc/sdvl_pose.hip equals the oracle, on inputs that
start at the identity and move by a few hundredths.

Measured 2026-10-18 over the 35 committed cases (the figures are printed by the tests, run with -s):
* Oracle against restatement: n_draws, both lists in order and refined are equal on every case.  The 4x4 poses differ by at most
  2.9e-14 (oblique-193-far, a start with metres of translation; 26 of the 34 cases stay below 1e-15).  POSE_BOUND is 100 times that,
  2.9e-12, and never more than 1e-10.  Nothing had to be resolved: the oracle does not depart from feature_align.cc on any case.
* The one-match case is pose_free: its normal equations have rank 2, the oracle's LDLT fills the null space from rounding (its
  pose moves by 1.6e-2 to 2.4e-1 under one ulp for all of the 11 seeds tried) and lstsq takes the minimum-norm step.  Decisions
  are equal; the poses are 3.8e-3 apart and the match lands 1.1e-16 apart, which is what is held (LANDING_BOUND).
* Branches taken, summed over the cases: rollback 1029, scale switch 1006, step-size stop 575, out of iterations 865,
  tmp < 1e-5 budget 45, budget of 0 4, rescue adds 27, rescue adds nothing 8, empty inlier set 1.
* The smallest relative distance of any tested error to its threshold, over all cases: 6.1e-6 (roll30-257).
* Admission screen: 3 seeds discarded (points2, seeds 1 to 3: n_draws or the lists change under one ulp), none among the
  outlier-heavy default cases, whose first seed passed.  Four seeds were chosen for what the case is there to show, not by the
  screen: optim0 (seed 2: no match within the threshold under the start pose), optim1 (3), nine (2) and seven-tight (5): the first
  whose tied or wrapped draws bear on the lists.
* Planted faults: cases of 34 (one-match left out) that separate each from the oracle: update_side 32, rotation_transposed 33,
  inv_cov_error_only 32, median_low 13, switch_at_4 25, rollback_keeps_current 21, rescue_1x 27, supporters_ge 3 (nine, optim0,
  optim1), window_no_wrap 2 (seven-tight, optim1), best_is_start 1 (optim0).
* The legacy inputs (make_matches as test_pose_from_matches_equals_oracle calls it; 11 of its 14 jobs, see the test) do NOT separate
  window_no_wrap and best_is_start.  They do separate the wrong-side update, by 3.3e-6 on the job of 150 matches, just over the
  1e-6 that counts here, where the new inputs give 8.3e-1 and different lists, and rollback_keeps_current by 1.4e-6.  The legacy
  job of 40 matches is itself balanced on a near-tie: the oracle moves its pose by 2.7e-9 when every ax moves one ulp down.
"""
import numpy as np
import pytest

from oraclelib import TUM_CAM, make_matches
from pose_cases import CASES, case, oracle_answer
from pose_restatement import BRANCHES, FAULTS, quat_to_rot, restate, se3_matrix

POSE_BOUND = 2.9e-12       # 100 x the largest oracle-to-restatement difference measured over the cases (2.9e-14), see above
assert POSE_BOUND <= 1e-10  # one order under the device bound of 1e-9, whatever is measured
STABLE_BOUND = 1e-12       # admission: the oracle's own movement under one-ulp perturbations
# a pose_free case (one match: the normal equations have rank 2 and the LDLT fills the null space from rounding) fixes where its
# match lands, not the pose.  Both ConvergePose calls of the case stop on the step size (max |dT| <= 1e-10, feature_align.cc:417):
# the residual left is at most the row sum of the Jacobian (< 3.2 for |x/z| <= 0.6, |y/z| <= 0.45, z >= 1.5) times that step, for
# each of the two poses compared: 2 * 3.2e-10 < 1e-9 in normalised image coordinates (5e-7 px).
LANDING_BOUND = 1e-9
# the case that is asserted to separate each planted fault from the oracle (any one would do; the docstring lists how many do)
WITNESS = {
    "update_side": "oblique-193-far", "rotation_transposed": "roll90-64", "inv_cov_error_only": "roll30-257",
    "median_low": "behind-100", "switch_at_4": "thr0.5", "rollback_keeps_current": "points8", "rescue_1x": "identity-150",
    "supporters_ge": "optim0", "window_no_wrap": "optim1", "best_is_start": "optim0",
}
LEGACY_SIZES = [(150, 40, 5, 3, 1, 0), (256, 255, 64, 65, 129, 7), (1024, 700, 257)]   # test_pose_from_matches_equals_oracle

_restated, _wanted = {}, {}


def wanted(orc, name):
    if name not in _wanted:
        _wanted[name] = oracle_answer(orc, case(name), TUM_CAM)
    return _wanted[name]


def restated(name, fault=None):
    if (name, fault) not in _restated:
        c = case(name)
        _restated[(name, fault)] = restate(c["obs"], c["pose"], TUM_CAM[0], c["rand_seed"], c["rand_skip"], fault=fault, **c["limits"])
    return _restated[(name, fault)]


def same_decisions(a, b):
    return (a["n_draws"] == b["n_draws"] and np.array_equal(a["inliers"], b["inliers"]) and np.array_equal(a["outliers"], b["outliers"])
            and a["refined"] == b["refined"])


def pose_distance(a, b):
    return float(np.abs(se3_matrix(a["pose"]) - se3_matrix(b["pose"])).max())


def landing(c, r):
    """where the case's inliers land under a result's pose, in normalised image coordinates"""
    pc = c["obs"][r["inliers"], 2:5] @ quat_to_rot(r["pose"][:4]).T + r["pose"][4:]
    return pc[:, :2] / pc[:, 2:3]


def separated(want, got):
    """the issue's measure: different lists, or a pose more than 1e-6 apart"""
    lists = not (np.array_equal(want["inliers"], got["inliers"]) and np.array_equal(want["outliers"], got["outliers"]))
    return lists or pose_distance(want, got) > 1e-6


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_is_stable_on_the_oracle(orc, name):
    """the admission screen of tests/pose_cases.py, run on every committed case: every start-pose component, and again every ax,
    moved one ulp up and one ulp down leaves n_draws, both lists and refined identical and the pose within 1e-12 (a pose_free case:
    where its match lands within LANDING_BOUND; the oracle's pose itself moves by 1.9e-2 there)"""
    c, w = case(name), wanted(orc, name)
    for sign in (1.0, -1.0):
        moved_pose = np.nextafter(c["pose"], sign * np.inf)
        moved_obs = c["obs"].copy()
        moved_obs[:, 0] = np.nextafter(moved_obs[:, 0], sign * np.inf)
        for what, v in (("start pose", oracle_answer(orc, c, TUM_CAM, pose=moved_pose)), ("ax", oracle_answer(orc, c, TUM_CAM, obs=moved_obs))):
            assert same_decisions(w, v), (name, what, sign, w["n_draws"], v["n_draws"])
            if c["pose_free"]:
                assert np.abs(landing(c, w) - landing(c, v)).max() <= LANDING_BOUND, (name, what, sign)
            else:
                assert pose_distance(w, v) <= STABLE_BOUND, (name, what, sign, pose_distance(w, v))


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_the_restatement(orc, name):
    c, w, r = case(name), wanted(orc, name), restated(name)
    assert w["n_draws"] == r["n_draws"], (w["n_draws"], r["n_draws"])
    assert np.array_equal(w["inliers"], r["inliers"]) and np.array_equal(w["outliers"], r["outliers"])
    assert w["refined"] == r["refined"]
    assert len(w["inliers"]) + len(w["outliers"]) == len(c["obs"])
    if c["pose_free"]:
        d = float(np.abs(landing(c, w) - landing(c, r)).max())
        print("%s: the match lands %.1e apart (normalised), poses %.1e apart" % (name, d, pose_distance(w, r)))
        assert d <= LANDING_BOUND
        return
    d = pose_distance(w, r)
    print("%s: n_draws %d, %d inliers, %d outliers, refined %d, pose %.1e from the restatement's, margin %.1e"
          % (name, w["n_draws"], len(w["inliers"]), len(w["outliers"]), w["refined"], d, r["trace"]["margin"]))
    assert d <= POSE_BOUND, d


def test_the_cases_reach_what_they_are_there_for(orc):
    """every branch of the trace is taken somewhere; jobs that stop after a handful of draws, jobs that go past draw 64, a budget
    of 0; the zero-threshold case leaves the rotated start pose alone"""
    total = dict.fromkeys(BRANCHES, 0)
    margin = np.inf
    for name in CASES:
        t = restated(name)["trace"]
        for k in BRANCHES:
            total[k] += t[k]
        margin = min(margin, t["margin"])
    print("branches over %d cases: %s; smallest relative distance of an error to its threshold %.1e" % (len(CASES), total, margin))
    for k in BRANCHES:
        assert total[k] > 0, k
    draws = {name: wanted(orc, name)["n_draws"] for name in CASES}
    assert min(draws.values()) == 1 and sum(1 for d in draws.values() if 1 < d < 10) >= 2, draws
    assert sum(1 for name, d in draws.items() if d > 64) >= 10 and draws["its129"] == 129, draws
    assert [draws[k] for k in ("its1", "its63", "its64", "its65")] == [1, 63, 64, 65]
    z = wanted(orc, "thr0")
    c = case("thr0")
    assert np.array_equal(z["pose"], c["pose"]) and z["refined"] == 0 and len(z["inliers"]) == 0
    assert np.array_equal(z["outliers"], np.arange(len(c["obs"])))
    levels = np.concatenate([case(n)["obs"][:, 5] for n in CASES])
    assert set(levels.astype(int)) == {0, 1, 2, 3, 4}
    b = case("behind-100")
    assert int(((b["obs"][:, 2:5] @ quat_to_rot(b["pose"][:4]).T + b["pose"][4:])[:, 2] < -0.4).sum()) == 4   # behind the start camera


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_case_separates_each_planted_fault(orc, fault):
    """the restatement with ONE error planted (pose_restatement.FAULTS) no longer agrees with the oracle on its witness case:
    the lists differ, or the pose is more than 1e-6 away.  Without the error the same case agrees (test above)."""
    name = WITNESS[fault]
    w, r = wanted(orc, name), restated(name, fault)
    print("%s on %s: lists %s, pose %.1e apart" % (fault, name, "differ" if not (np.array_equal(w["inliers"], r["inliers"]) and np.array_equal(
        w["outliers"], r["outliers"])) else "equal", pose_distance(w, r)))
    assert separated(w, r), (fault, name)


def test_which_faults_the_legacy_inputs_separate(orc):
    """The same faults over the inputs the stage was tested with so far: make_matches with the sizes, seeds, outlier shares and
    rand positions of test_gpu_parity.py::test_pose_from_matches_equals_oracle.  A job counts only where the restatement WITHOUT a
    fault agrees with the oracle (the jobs of 1, 3 and 5 matches do not: there the pose, or the draw it stops at, hangs on the
    solver's treatment of a nearly singular system).  Recorded in the module docstring, not asserted, except that the list of
    missed faults must not be empty while the wrong-side update is among them."""
    jobs = []
    for sizes in LEGACY_SIZES:
        for j, n in enumerate(sizes):
            if n == 0:
                continue
            obs, guess = make_matches(orc, n, seed=100 + j, outlier_frac=0.1 + 0.1 * (j % 4))
            w = orc.pose_from_matches(TUM_CAM, obs, guess, rand_seed=3, rand_skip=17 * j)
            r = restate(obs, guess, TUM_CAM[0], 3, 17 * j)
            if same_decisions(w, r) and pose_distance(w, r) <= POSE_BOUND:
                jobs.append((n, obs, guess, 17 * j, w))
    print("legacy jobs on which the restatement agrees with the oracle: %s" % [j[0] for j in jobs])
    assert len(jobs) >= 10
    missed = []
    for fault in FAULTS:
        hit = None
        for n, obs, guess, skip, w in jobs:
            r = restate(obs, guess, TUM_CAM[0], 3, skip, fault=fault)
            if separated(w, r):
                hit = (n, pose_distance(w, r))
                break
        print("%s: %s" % (fault, "separated by the job of %d matches (pose %.1e apart)" % hit if hit else "NOT separated by any legacy job"))
        if hit is None:
            missed.append(fault)
    print("faults the legacy inputs miss: %s" % missed)
    if "update_side" in missed:
        assert missed
