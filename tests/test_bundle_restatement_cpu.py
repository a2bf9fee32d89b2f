"""tests/bundle_restatement.py against itself and against the ground truth of tests/bundle_cases.py: the specification of
sdvl_bundle_adjust has to be right before a device result is compared with it (tests/test_gpu_bundle.py).

The ground-truth test.  From the cases' own starts (poses 4e-3, points 2e-2 off) with exact observations the minimum is the truth, and
the restatement run to convergence must find it: pose entries within 1e-6, point coordinates within 1e-6 of the scene depth.  Bundle::Local's
5 + 10 iterations do not converge from there: lambda starts every stage at 1e-5 max |H_jj| (about 1e3 for `full`, whose pose blocks sum
700 edges) and falls by at most 3 per accepted step, while the depth of a point seen from two neighbouring keyframes has a curvature
of 10 - 100.  So the test runs the same code with 40 stage-2 iterations (it stops by itself after 25 - 32), and prints what 5 + 10 reach
(`full`: 4.5e-6 / 4.1e-3 from the truth; chi2 falls from 9.9 to 1.5e-4).  With one fixed camera (`pair`, `triple`) the scale of the scene is a
gauge freedom that lambda alone holds: the converged result is the truth scaled about the fixed camera's centre by 1.0014 / 0.9986, and
is compared after that one scale (least squares over the points) is taken out; without it `pair` ends 4.3e-4 / 8.6e-3 from the truth at
chi2 = 1e-26."""
import math

import numpy as np
import pytest

import bundle_cases as bc
import bundle_restatement as br

CONVERGED_ITS = (5, 40)


def test_edge_jacobians_match_central_differences():
    p = bc.case("triple")
    poses, points = np.array(p["poses"]), np.array(p["points"])
    err0, _, Ji, Jj = br.edge_terms(poses, points, p["edge_pt"], p["edge_kf"], p["edge_uv"], p["cam"])
    h = 1e-6
    for e in range(0, len(err0), 5):
        pt, kf = p["edge_pt"][e], p["edge_kf"][e]
        sel = (p["edge_pt"][e:e + 1], p["edge_kf"][e:e + 1], p["edge_uv"][e:e + 1], p["cam"])
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            lo, hi = points.copy(), points.copy()
            lo[pt] -= d
            hi[pt] += d
            num = (br.edge_terms(poses, hi, *sel, jac=False)[0][0] - br.edge_terms(poses, lo, *sel, jac=False)[0][0]) / (2 * h)
            assert np.allclose(num, Ji[e][:, c], rtol=1e-6, atol=1e-5), (e, c)
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            lo, hi = poses.copy(), poses.copy()
            lo[kf] = br.exp_update(poses[kf], -d)
            hi[kf] = br.exp_update(poses[kf], d)
            num = (br.edge_terms(hi, points, *sel, jac=False)[0][0] - br.edge_terms(lo, points, *sel, jac=False)[0][0]) / (2 * h)
            assert np.allclose(num, Jj[e][:, c], rtol=1e-6, atol=1e-5), (e, c)


@pytest.mark.parametrize("name", ["triple", "single", "outliers"])
def test_schur_step_equals_the_full_system(name):
    """one damped step through the Schur complement = numpy.linalg.solve on the full (poses + points) system"""
    p = bc.case(name)
    poses, points = np.array(p["poses"]), np.array(p["points"])
    active = np.ones(len(p["edge_pt"]), bool)
    s = br.System(p, poses, points, active, True)
    lam = 1e-5 * s.max_diagonal() * 37.0
    dp, dl, scale = s.solve(lam)
    nf, npt = s.n_free, s.n_pt
    n = 6 * nf + 3 * npt
    H, b = np.zeros((n, n)), np.concatenate([s.bp.reshape(-1), s.bl.reshape(-1)])
    for a in range(nf):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = s.Hpp[a]
    for q in range(npt):
        o = 6 * nf + 3 * q
        H[o:o + 3, o:o + 3] = s.Hll[q]
    for W, a, q in zip(s.W, s.f_kf, s.f_pt):
        o = 6 * nf + 3 * q
        H[6 * a:6 * a + 6, o:o + 3] += W
        H[o:o + 3, 6 * a:6 * a + 6] += W.T
    x = np.linalg.solve(H + lam * np.eye(n), b)
    ref = np.abs(x).max()
    assert np.abs(x[:6 * nf] - dp.reshape(-1)).max() <= 1e-9 * ref
    assert np.abs(x[6 * nf:] - dl.reshape(-1)).max() <= 1e-9 * ref
    assert abs(scale - float(x @ (lam * x + b))) <= 1e-9 * abs(scale)


def rescale_about(poses, points, fixed_pose, truth_points):
    """the scene scaled about the fixed camera's centre (its pose unchanged) by the least-squares scale onto the true points"""
    c0 = -br.quat_to_rot(fixed_pose[:4])[0].T @ fixed_pose[4:]
    a, b = points - c0, truth_points - c0
    s = float(np.sum(a * b) / np.sum(a * a))
    out = poses.copy()
    for k in range(len(poses)):
        R = br.quat_to_rot(poses[k, :4])[0]
        out[k, 4:] = -R @ (c0 + s * (-R.T @ poses[k, 4:] - c0))
    return out, c0 + s * a, s


@pytest.mark.parametrize("name", ["pair", "triple", "full"])
def test_exact_observations_recover_the_truth(name):
    p = bc.case(name, noise=0.0)
    depth = float(np.median(p["truth_points"][:, 2]))
    short = br.bundle_adjust(p)
    print("%s after 5 + 10: pose %.3g point %.3g, chi2 %.3g -> %.3g" % (name, np.abs(short["poses"] - p["truth_poses"]).max(),
          np.abs(short["points"] - p["truth_points"]).max(), short["stages"][0]["chi2_before"], short["stages"][1]["chi2_after"]))
    assert short["stages"][1]["chi2_after"] <= 1e-3 * short["stages"][0]["chi2_before"]
    r = br.bundle_adjust(p, CONVERGED_ITS)
    assert r["status"] == br.OK and r["n_level1"] == 0 and r["stages"][1]["iterations"] < CONVERGED_ITS[1]
    poses, points, scale = r["poses"], r["points"], 1.0
    if name in ("pair", "triple"):
        poses, points, scale = rescale_about(poses, points, p["truth_poses"][p["n_free"]], p["truth_points"])
    d_pose = np.abs(poses - p["truth_poses"]).max()
    d_pt = np.abs(points - p["truth_points"]).max()
    print("%s converged (%d stage-2 iterations, scale %.6f): pose %.3g point %.3g (scene depth %.1f)"
          % (name, r["stages"][1]["iterations"], scale, d_pose, d_pt, depth))
    assert d_pose <= 1e-6
    assert d_pt <= 1e-6 * depth


def test_outliers_end_at_level_one_exactly():
    p, r = bc.case("outliers"), bc.restated("outliers")
    assert p["shifted"].sum() == len(p["shifted"]) // 10
    assert np.array_equal(r["levels"] == 1, p["shifted"])
    assert r["stages"][1]["chi2_before"] < r["stages"][0]["chi2_after"]       # stage 2 runs without them


def test_cases_exercise_what_they_are_for():
    r = bc.restated("dropped")
    assert list(r["pose_stages"]) == [3, 3, 0, 3]
    r = bc.restated("behind")
    assert r["n_level1"] > 0 and max(r["stages"][0]["trials_per_it"]) >= 3
    assert np.sum(r["point_stages"] != 3) >= 1
    r = bc.restated("rejects")                   # several trials per iteration, in more than one iteration, in both stages
    assert sum(q >= 3 for q in r["stages"][0]["trials_per_it"]) >= 2 and sum(q >= 2 for q in r["stages"][1]["trials_per_it"]) >= 2
    assert r["n_level1"] == 0
    assert bc.restated("full")["stages"][0]["iterations"] == 5
    for name in bc.NAMES:
        r = bc.restated(name)
        assert r["status"] == br.OK
        for s in r["stages"]:
            assert s["chi2_after"] <= s["chi2_before"]


@pytest.mark.parametrize("name", bc.NAMES)
def test_margins_that_make_the_device_comparison_meaningful(name):
    """every edge at least 1e-6 away from 5.991 and from z = 0 at the classification point; every accept / reject decision before
    the first settled trial holds when chi' moves by +-1e-9 chi"""
    p, r = bc.case(name), bc.restated(name)
    # the classification point: the estimates stage 1 ended on = the state stage 2 started from; recover it by running stage 1 alone
    poses, points, _ = br.run_stage(p, np.array(p["poses"]), np.array(p["points"]), np.ones(len(p["edge_pt"]), bool), True, 5, [], 0)
    err, z, _, _ = br.edge_terms(poses, points, p["edge_pt"], p["edge_kf"], p["edge_uv"], p["cam"], jac=False)
    assert np.abs(np.sum(err * err, 1) - br.CHI2_TH).min() >= 1e-6
    assert np.abs(z).min() >= 1e-6
    for t in r["log"]:
        if t["settled"]:
            break
        for sign in (-1.0, 1.0):
            assert br.decide(t["chi"], t["chi_new"] + sign * 1e-9 * t["chi"], t["scale"], t["ok"])[1] == t["accepted"], t


def test_statuses_of_degenerate_problems():
    p = dict(bc.case("pair"))
    e = dict(p, poses=np.zeros((0, 7)), fixed=np.zeros(0, np.int32), edge_pt=np.zeros(0, np.int32), edge_kf=np.zeros(0, np.int32),
             edge_uv=np.zeros((0, 2)))
    assert br.bundle_adjust(e)["status"] == br.EMPTY
    e = dict(p, edge_pt=np.zeros(0, np.int32), edge_kf=np.zeros(0, np.int32), edge_uv=np.zeros((0, 2)))
    assert br.bundle_adjust(e)["status"] == br.NO_EDGES
    uv = np.array(p["edge_uv"])
    uv[3, 0] = math.nan
    r = br.bundle_adjust(dict(p, edge_uv=uv))
    assert r["status"] == br.NONFINITE and np.array_equal(r["poses"], p["poses"]) and np.array_equal(r["points"], p["points"])
