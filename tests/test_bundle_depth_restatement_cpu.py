"""tests/bundle_depth_restatement.py against itself, against tests/bundle_restatement.py and against the ground truth of
tests/bundle_depth_cases.py: the specification of sdvl_bundle_adjust_depth has to be right before a device result is compared with it
(tests/test_gpu_bundle_depth.py).

`scale`.  With one fixed keyframe the scale of a monocular map is a gauge freedom: the truth scaled by 1.05 about the fixed keyframe's
centre has chi2 = 0, and the monocular restatement leaves it there, 0.3 from the truth.  A depth on the edges is metric: the depth
restatement returns to the truth.  The bounds (monocular end error >= 0.29; depth end error <= 1e-9 with a depth on every edge,
<= 1e-5 with one on half of them) are the conditions of the issue this file was written for, set from its float64 prototype (3e-15,
and 2.3e-7 / 4.2e-13 on the half shares)."""
import numpy as np
import pytest

import bundle_cases as bc
import bundle_depth_cases as dc
import bundle_depth_restatement as bd
import bundle_restatement as br


def test_edge_jacobians_match_central_differences():
    p = dc.case("triple/half")
    poses, points = np.array(p["poses"]), np.array(p["points"])
    assert (p["edge_d"] > 0).any() and (p["edge_d"] == 0).any()
    err0, _, Ji, Jj = bd.edge_terms(poses, points, p["edge_pt"], p["edge_kf"], p["edge_uv"], p["edge_d"], p["cam"], p["bf"])
    assert not Ji[p["edge_d"] == 0, 2].any() and not Jj[p["edge_d"] == 0, 2].any() and not err0[p["edge_d"] == 0, 2].any()
    h = 1e-6
    for e in range(0, len(err0), 3):
        pt, kf = p["edge_pt"][e], p["edge_kf"][e]
        sel = (p["edge_pt"][e:e + 1], p["edge_kf"][e:e + 1], p["edge_uv"][e:e + 1], p["edge_d"][e:e + 1], p["cam"], p["bf"])
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            lo, hi = points.copy(), points.copy()
            lo[pt] -= d
            hi[pt] += d
            num = (bd.edge_terms(poses, hi, *sel, jac=False)[0][0] - bd.edge_terms(poses, lo, *sel, jac=False)[0][0]) / (2 * h)
            assert np.allclose(num, Ji[e][:, c], rtol=1e-6, atol=1e-5), (e, c)
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            lo, hi = poses.copy(), poses.copy()
            lo[kf] = br.exp_update(poses[kf], -d)
            hi[kf] = br.exp_update(poses[kf], d)
            num = (bd.edge_terms(hi, points, *sel, jac=False)[0][0] - bd.edge_terms(lo, points, *sel, jac=False)[0][0]) / (2 * h)
            assert np.allclose(num, Jj[e][:, c], rtol=1e-6, atol=1e-5), (e, c)


@pytest.mark.parametrize("name", bc.NAMES)
def test_without_a_depth_it_is_the_monocular_restatement(name):
    p = bc.case(name)
    got = bd.bundle_adjust(dict(p, edge_d=np.zeros(len(p["edge_pt"])), bf=dc.BF))
    ref = bc.restated(name)
    assert got["status"] == ref["status"] and got["n_level1"] == ref["n_level1"]
    for k in ("poses", "points", "levels", "pose_stages", "point_stages"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["stages"] == ref["stages"]
    assert got["log"] == ref["log"]


@pytest.mark.parametrize("src", ["pair", "triple"])
def test_scale_is_a_gauge_freedom_only_without_depth(src):
    truth = bc.case(src)["truth_points"]
    p = dc.scale(src, "all")
    mono = br.bundle_adjust(p)
    d_mono = float(np.abs(mono["points"] - truth).max())
    print("%s monocular: chi2 %.3g -> %.3g, point error %.3g" % (src, mono["stages"][0]["chi2_before"], mono["stages"][1]["chi2_after"], d_mono))
    assert d_mono >= 0.29
    for share, bound in (("all", 1e-9), ("half", 1e-5)):
        p = dc.scale(src, share)
        r = bd.bundle_adjust(p)
        d = max(float(np.abs(r["points"] - truth).max()), float(np.abs(r["poses"] - p["truth_poses"]).max()))
        print("%s depth on %s: chi2 %.3g -> %.3g, error %.3g" % (src, share, r["stages"][0]["chi2_before"], r["stages"][1]["chi2_after"], d))
        assert r["status"] == br.OK and r["n_level1"] == 0
        assert d <= bound


def test_wrong_depths_end_at_level_one():
    p, r = dc.case("wrong_depth"), dc.restated("wrong_depth")
    wrong, shifted, lv = p["wrong"], p["shifted"], r["levels"] == 1
    clean = ~wrong & ~shifted
    print("wrong depths %d, on level 1 %d; clean edges on level 1 %d; shifted on level 1 %d of %d"
          % (wrong.sum(), (lv & wrong).sum(), (lv & clean).sum(), (lv & shifted).sum(), shifted.sum()))
    assert wrong.sum() == len(wrong) // 10
    assert lv[wrong].all()
    assert (lv & clean).sum() <= 2
    assert lv[shifted].all()


def test_cases_exercise_what_they_are_for():
    for name in dc.NAMES:
        p, r = dc.case(name), dc.restated(name)
        has = p["edge_d"] > 0
        assert r["status"] == br.OK, name
        assert has.all() if not name.endswith("/half") else (has.sum() == len(has) // 2), name
        for s in r["stages"]:
            assert s["chi2_after"] <= s["chi2_before"], name
    # the depth perturbation is 0.5 px of disparity: the third residual at the truth has that spread
    p = dc.case("full/all")
    z = dc.true_z(p)
    sd = float(np.std(p["bf"] / p["edge_d"] - p["bf"] / z))
    assert 0.45 <= sd <= 0.55, sd
    assert list(dc.restated("dropped/all")["pose_stages"]) == [3, 3, 0, 3]
    assert dc.restated("behind/all")["n_level1"] > 0


def margins(name):
    """-> the smallest relative distance of an edge's chi2 to its threshold and the smallest |z| at the classification point"""
    p = dc.case(name)
    poses, points, _ = bd.run_stage(p, np.array(p["poses"]), np.array(p["points"]), np.ones(len(p["edge_pt"]), bool), True, 5, [], 0)
    err, z, _, _ = bd.edge_terms(poses, points, p["edge_pt"], p["edge_kf"], p["edge_uv"], p["edge_d"], p["cam"], p["bf"], jac=False)
    th = bd.thresholds(p["edge_d"])
    return float((np.abs(bd.chi2_rows(err) - th) / th).min()), float(np.abs(z).min())


@pytest.mark.parametrize("name", dc.NAMES)
def test_margins_that_make_the_device_comparison_meaningful(name):
    """every edge at least 1e-6 away from its threshold and from z = 0 at the classification point; every accept / reject decision
    before the first settled trial holds when chi' moves by +-1e-9 chi"""
    m_chi, m_z = margins(name)
    r = dc.restated(name)
    n_settled = sum(t["settled"] for t in r["log"])
    print("%s: margin to the threshold %.3g (relative), |z| >= %.3g, settled trials %d of %d" % (name, m_chi, m_z, n_settled, len(r["log"])))
    assert m_chi >= 1e-6
    assert m_z >= 1e-6
    for t in r["log"]:
        if t["settled"]:
            break
        for sign in (-1.0, 1.0):
            assert br.decide(t["chi"], t["chi_new"] + sign * 1e-9 * t["chi"], t["scale"], t["ok"])[1] == t["accepted"], t
