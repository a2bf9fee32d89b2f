"""The device pose stage (csrc/sdvl_pose.hip: pose_hypotheses_kernel, pose_hypotheses_wave_kernel, pose_refine_kernel<1> and <3>)
against the oracle on the named cases of tests/pose_cases.py, each case in every launch form the dispatch has, and with every limit
away from its default.  The oracle is itself held against an independent restatement of the reference on the same cases
(tests/test_oracle_pose_independent.py).

Acceptance is that of the four pose tests of tests/test_gpu_parity.py: n_draws, both lists in order and refined equal the oracle's,
the pose is within 1e-9 (the device's sin and cos inside SE3::Exp differ from libm's by an ulp).

The dispatch (sdvl_pose_enqueue_device) picks the form from the number of jobs and the largest job of a call:
  csrc/sdvl_pose.hip:759  wave_form = batch_size <= 4          one wave per draw, else one lane per draw with only the first 64
                                                                draws converged ahead and the rest on demand in pose_refine
  csrc/sdvl_pose.hip:774  max_obs > 256 || batch_size <= 32     pose_refine_kernel<3> (helper waves), else pose_refine_kernel<1>
                                                                with its 256-entry LDS lists
Both forms of a pair carry the same kernel timer name, so each test restates the condition it aims at and asserts it on its batch.

A call has ONE set of limits.  A case with limits of its own is therefore batched with the inputs of other cases run under ITS
limits; those fillers shape the launch and are not compared (the oracle was not screened for stability on them under foreign
limits, and the stage is chaotic on jobs balanced on a near-tie).  Every job of a batch whose own limits are the batch's is compared.

Measured 2026-10-18 on one MI355X, 35 cases: the device agrees with the oracle on every case in every form; the module's 15 tests
take 3.0 s, of which 1.6 s open the context."""
import importlib

import numpy as np
import pytest

from oraclelib import TUM_CAM, quat_rot
from pose_cases import CASES, DEFAULT_CASES, DEFAULTS, PARAM_CASES, case, oracle_answer

pytestmark = pytest.mark.gpu

POSE_BOUND = 1e-9
LANDING_BOUND = 1e-9     # a pose_free case: where its match lands, in normalised image coordinates; derived in test_oracle_pose_independent.py
FILLERS = [n for n in DEFAULT_CASES if len(case(n)["obs"]) <= 256]
assert len(FILLERS) >= 12 and "roll90-256" in FILLERS

_wanted = {}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


def wanted(orc, name):
    """the oracle's answer to a case under its own limits, computed once and shared (read-only)"""
    if name not in _wanted:
        _wanted[name] = oracle_answer(orc, case(name), TUM_CAM)
    return _wanted[name]


def forms_of(names):
    """(wave_form, three_wave_refine) of a call with these jobs, as csrc/sdvl_pose.hip:759 and :774 compute them"""
    batch_size, max_obs = len(names), max(len(case(n)["obs"]) for n in names)
    return batch_size <= 4, (max_obs > 256 or batch_size <= 32)


def run(ctx, orc, names, limits):
    jobs = []
    for n in names:
        c = case(n)
        draws = orc.rand_stream(c["rand_skip"] + limits["max_ransac_its"], seed=c["rand_seed"])[c["rand_skip"]:]
        jobs.append((c["obs"], c["pose"], draws))
    return ctx.pose_from_matches(jobs, fx=TUM_CAM[0], **limits)


def landing(c, r):
    pc = c["obs"][r["inliers"], 2:5] @ quat_rot(r["pose"][:4]).T + r["pose"][4:]
    return pc[:, :2] / pc[:, 2:3]


def differences(orc, name, g):
    """-> what differs between the device's answer and the oracle's on a case, as a list of strings (empty: accepted)"""
    c, w = case(name), wanted(orc, name)
    bad = []
    if g["n_draws"] != w["n_draws"]:
        bad.append("n_draws %d != %d" % (g["n_draws"], w["n_draws"]))
    if not np.array_equal(g["inliers"], w["inliers"]):
        bad.append("inliers differ (%d, %d)" % (len(g["inliers"]), len(w["inliers"])))
    if not np.array_equal(g["outliers"], w["outliers"]):
        bad.append("outliers differ (%d, %d)" % (len(g["outliers"]), len(w["outliers"])))
    if g["refined"] != w["refined"]:
        bad.append("refined %d != %d" % (g["refined"], w["refined"]))
    if c["pose_free"]:
        if not bad and np.abs(landing(c, g) - landing(c, w)).max() > LANDING_BOUND:
            bad.append("lands %.2e away" % np.abs(landing(c, g) - landing(c, w)).max())
    elif np.abs(g["pose"] - w["pose"]).max() > POSE_BOUND:
        bad.append("pose %.2e away" % np.abs(g["pose"] - w["pose"]).max())
    return ["%s: %s" % (name, b) for b in bad]


def batch_around(name, size, fillers):
    """`size` job names: the case in the middle, the fillers (the case itself left out) cycled around it"""
    pool = [f for f in fillers if f != name]
    k = list(CASES).index(name)                     # a different rotation of the fillers for each case
    rest = [pool[(k + i) % len(pool)] for i in range(size - 1)]
    return rest[:size // 2] + [name] + rest[size // 2:]


def check_batches(ctx, orc, names, size, fillers, want_forms, must_hold=()):
    """each named case in a batch of `size`; every job whose own limits are the batch's is compared with the oracle"""
    bad, compared = [], 0
    for name in names:
        batch = batch_around(name, size, fillers)
        assert all(m in batch for m in must_hold), (name, must_hold)
        assert forms_of(batch) == want_forms, (name, forms_of(batch))
        limits = case(name)["limits"]
        got = run(ctx, orc, batch, limits)
        for n, g in zip(batch, got):
            if case(n)["limits"] == limits:
                bad += ["[batch of %s] %s" % (name, d) for d in differences(orc, n, g)]
                compared += 1
    assert not bad, bad
    return compared


# ------------------------------------------------------------------------------------------------ every case in every form
def test_every_case_alone(ctx, orc):
    """batch_size 1 <= 4: pose_hypotheses_wave_kernel (sdvl_pose.hip:759); batch_size <= 32: pose_refine_kernel<3> (:774), also for
    the jobs of 1 to 9 matches that leave the helper waves nothing to do"""
    for name in CASES:
        assert forms_of([name]) == (True, True)
    bad = []
    for name in CASES:
        bad += differences(orc, name, run(ctx, orc, [name], case(name)["limits"])[0])
    assert not bad, bad


def test_every_case_in_a_batch_of_4(ctx, orc):
    """batch_size 4 <= 4: still the wave form (:759), four jobs of different sizes behind one grid; pose_refine_kernel<3> (:774)"""
    assert check_batches(ctx, orc, list(CASES), 4, FILLERS, (True, True)) >= len(CASES)


@pytest.mark.parametrize("size", [5, 32])
def test_every_case_in_the_lane_form_with_helper_waves(ctx, orc, size):
    """batch_size 5 > 4: pose_hypotheses_kernel, one lane per draw (:759-769); 5 and 32 <= 32: pose_refine_kernel<3> (:774), counting
    the supporters as its replay reaches a draw and converging draws past 64 on demand"""
    assert check_batches(ctx, orc, list(CASES), size, FILLERS, (False, True)) >= len(CASES)


def test_every_case_up_to_256_matches_in_the_one_wave_refine(ctx, orc):
    """batch_size 33 > 32 and max_obs == 256 exactly, not above: pose_refine_kernel<1> with its 256-entry LDS lists (:774-779).
    The four cases above 256 matches cannot reach this form; the 256-match case is in every batch."""
    names = [n for n in CASES if len(case(n)["obs"]) <= 256]
    assert len(names) == len(CASES) - 4
    assert check_batches(ctx, orc, names, 33, FILLERS, (False, False), must_hold=["roll90-256"]) >= len(names)


def test_every_case_in_a_batch_of_33_with_one_job_of_257(ctx, orc):
    """batch_size 33 > 32 but one job of 257 matches: max_obs > 256 sends the WHOLE batch to pose_refine_kernel<3> (:774)"""
    fillers = FILLERS + ["roll30-257"]
    names = [n for n in CASES if n != "roll30-257"]
    assert check_batches(ctx, orc, names, 33, fillers, (False, True), must_hold=["roll30-257"]) >= len(names)
    batch = batch_around("roll30-257", 33, FILLERS)              # and the 257-match case itself among 32 jobs of at most 256
    assert forms_of(batch) == (False, True)
    got = run(ctx, orc, batch, DEFAULTS)
    bad = [d for n, g in zip(batch, got) for d in differences(orc, n, g)]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the limits
@pytest.mark.parametrize("size", [6, 40])
def test_limits_away_from_their_defaults(ctx, orc, size):
    """max_ransac_points 1, 2, 8; max_ransac_its 1, 63, 64, 65, 129; max_optim_pose_its 0, 1, 5, 6; thresholds 0, 0.5, 8 px: in the
    lane form with the helper waves (6 jobs) and with the one-wave refine (40 jobs of at most 256 matches), so that 63, 64, 65 and 129
    draws meet both the 64 draws converged ahead (kHypDraws) and the ones converged on demand, and the lane form's LDS cache is
    sized by 1, 2 and 8 points"""
    assert {case(n)["limits"][k] for n in PARAM_CASES for k in ("max_ransac_points",)} >= {1, 2, 8}
    assert {case(n)["limits"]["max_ransac_its"] for n in PARAM_CASES} >= {1, 63, 64, 65, 129}
    assert {case(n)["limits"]["max_optim_pose_its"] for n in PARAM_CASES} >= {0, 1, 5, 6}
    assert {case(n)["limits"]["inlier_error_threshold"] for n in PARAM_CASES} >= {0.0, 0.5, 8.0}
    check_batches(ctx, orc, PARAM_CASES, size, FILLERS, (False, size <= 32))
    draws = [wanted(orc, n)["n_draws"] for n in PARAM_CASES]
    assert max(draws) > 64 and min(draws) < 10, draws             # on-demand draws and an early stop are both among them


@pytest.mark.parametrize("size", [1, 6])
def test_zero_threshold_from_a_rotated_start(ctx, orc, size):
    """No draw has a supporter at a threshold of 0, so the matches are classified with a default-constructed SE3
    (feature_align.cc:159, :215; `Rigid best = se3_identity()` on the device), which from an identity start could not be told from
    the start pose.  From a start rolled by 90 degrees: the start pose comes back unchanged, bit for bit, every match is an outlier
    in index order, all 100 draws are made and refined is 0."""
    c = case("thr0")
    batch = batch_around("thr0", size, FILLERS)
    g = run(ctx, orc, batch, c["limits"])[batch.index("thr0")]
    assert np.array_equal(g["pose"], c["pose"]) and g["refined"] == 0 and g["n_draws"] == 100
    assert len(g["inliers"]) == 0 and np.array_equal(g["outliers"], np.arange(len(c["obs"])))
    assert not differences(orc, "thr0", g)


@pytest.mark.parametrize("size", [1, 6, 40])
def test_rank_deficient_hypotheses(ctx, orc, size):
    """max_ransac_points 1 and 2 (every hypothesis solves a system of rank 2 or 4) and a job of one match: n_draws, the lists and
    refined are exact.  The FINAL pose of the two big jobs comes from all their inliers and is well determined: the oracle moves
    it by 2.2e-16 and 3.3e-16 under the one-ulp perturbations of the admission screen, so it is held to 1e-9 like any other.  The
    one-match job's final system has rank 2 itself: the oracle moves its pose by 1.9e-2 under those perturbations, and the device's
    null-space fill is its own; what is determined is where the match lands (LANDING_BOUND), as for the single-feature
    alignment of tests/test_gpu_forms.py."""
    bad = []
    for name in ("points1", "points2", "one-match"):
        assert case(name)["rank_deficient"]
        batch = batch_around(name, size, FILLERS)
        g = run(ctx, orc, batch, case(name)["limits"])[batch.index(name)]
        bad += differences(orc, name, g)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ a batch equals each job alone
@pytest.mark.parametrize("names", [["nine", "roll90-64", "one-match", "oblique-192"],
                                   ["roll30-63", "five", "oblique-193-far", "repeated-40", "roll90-256", "six", "behind-100", "near-120"]],
                         ids=["wave-form", "lane-form"])
def test_a_batch_equals_each_job_alone(ctx, orc, names):
    """a job's answer does not depend on its neighbours, nor on the form its hypotheses were made in: n_draws, lists, refined and the
    bits of the pose of a job in a mixed batch (the wave form for 4 jobs, the lane form for 8: :759) equal those of the job in a call
    of its own.  (The final pose is pose_refine_kernel<3>'s in all these calls and depends on the hypotheses only through the lists.)"""
    assert forms_of(names) == (len(names) <= 4, True)
    together = run(ctx, orc, names, DEFAULTS)
    for n, t in zip(names, together):
        a = run(ctx, orc, [n], DEFAULTS)[0]
        assert a["n_draws"] == t["n_draws"] and a["refined"] == t["refined"], n
        assert np.array_equal(a["inliers"], t["inliers"]) and np.array_equal(a["outliers"], t["outliers"]), n
        assert np.array_equal(a["pose"], t["pose"]), n
