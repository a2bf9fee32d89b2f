"""The restatement of the depth filter with a measured depth (tests/depth_measure_restatement.py, the specification of
sdvl_depth_filter_measured) on the designed cases of tests/depth_measure_cases.py: every case goes where its name says; a measured case
returns the range of the point its sample measures; a request that does not measure IS depth_restatement's; every planted fault changes a
case; the lookup agrees with depth_seed_restatement where the two rules meet (whole-numbered positions).  No GPU."""
import math

import numpy as np
import pytest

import depth_measure_cases as mc
import depth_measure_restatement as dm
import depth_restatement as dr
import depth_seed_restatement as dsr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED

CASES = mc.all_cases()
NAMES = [c["name"] for c in CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_says(name):
    mc.check(mc.by_name(name))


def test_cases_reach_what_the_device_test_needs():
    got = {c["name"]: dm.restate(**mc.inputs(c)) for c in CASES}
    measured = [c for c in CASES if got[c["name"]]["status"] == dsr.OK]
    assert {c["level"] for c in measured} == {0, 1, 2, 3, 4}
    assert {got[c["name"]]["status"] for c in CASES} == {dsr.OK, dsr.HOLE, dsr.FEW, dsr.EDGE, dsr.OUTSIDE, dm.NO_LOOKUP}
    assert {got[c["name"]]["outcome"] for c in CASES} == {NOT_FOUND, NOT_FOUND | DELETED, SKIPPED, UPDATED, CONVERGED, FIXED_STALE}
    assert {c["depth"].dtype for c in measured} == {np.dtype(np.float32), np.dtype(np.uint16)}
    assert any(c["dist"] is not None for c in measured) and any(c["dist"] is None for c in measured)
    assert {c["layout"] for c in measured if c["depth"].dtype == np.uint16} == {"odd", "padded", "tight"}
    assert any(c["state"]["fixed"] for c in measured)
    assert any(c["depth"] is None and c["found"] for c in CASES)
    outcomes = {got[c["name"]]["outcome"] for c in measured}
    assert outcomes == {SKIPPED, UPDATED, CONVERGED}
    # strides of 8 and 16 push neighbours off the 24 x 16 image
    for c in measured:
        if c["level"] >= 3:
            fu, fv = dm.centre(c["px"], c["cam"], c["dist"])
            s = 1 << c["level"]
            assert fu + s >= mc.W or fu - s < 0 or fv + s >= mc.H or fv - s < 0


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["want"].get("exact_range")])
def test_true_depth_gives_the_true_range(name):
    """the sample is the z of a point on the candidate's ray: the restatement's depth is that point's range, and a prior centred on it
    stays there"""
    c = mc.by_name(name)
    o = dm.restate(**mc.inputs(c))
    assert o["status"] == dsr.OK
    assert abs(o["trace"]["depth"] - c["range"]) <= 1e-12 * c["range"], (o["trace"]["depth"], c["range"])
    assert abs(o["trace"]["x"] - 1.0 / c["range"]) <= 2e-12 / c["range"]
    # and tau is the stated noise of the sample, not of the range
    z = o["trace"]["z"]
    assert o["trace"]["tau"] == mc.NOISE["noise_abs"] + mc.NOISE["noise_quad"] * (z * z)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if dm.restate(**mc.inputs(c))["status"] != dsr.OK])
def test_not_measured_is_the_triangulated_restatement(name):
    c = mc.by_name(name)
    o = dm.restate(**mc.inputs(c))
    want = dr.restate(**mc.triangulated_inputs(c))
    got = {k: v for k, v in o.items() if k != "status"}
    assert repr(got) == repr(want)                      # (repr: NaN compares unequal to itself)
    # and its bound is that rule's bound
    assert dm.tolerance(**mc.inputs(c))[1] == dr.tolerance(**mc.triangulated_inputs(c))[1]


def _changed(c, fault):
    a, b = dm.restate(**mc.inputs(c)), dm.restate(fault=fault, **mc.inputs(c))
    keys = ("status", "outcome", "n_failed", "rho", "sigma2", "a", "b", "cos_alpha", "last_distance", "position", "row")
    return repr([a[k] for k in keys]) != repr([b[k] for k in keys])


@pytest.mark.parametrize("fault", sorted(dm.FAULTS))
def test_every_fault_changes_a_case(fault):
    hit = [c["name"] for c in CASES if _changed(c, fault)]
    print("%s: %d cases change (%s)" % (fault, len(hit), ", ".join(hit[:6])))
    assert hit, (fault, dm.FAULTS[fault])


def test_faults_named_by_design():
    """the cases built for a fault are among those it changes"""
    for fault, name in (("stride_level0", "few-level4"), ("stride_level0", "edge-stride4"), ("centre_truncated", "ok-01-level0"),
                        ("parallax_kept", "ok-no-parallax"), ("no_depth_mean_test", "skip-depth_mean"), ("negative_depth_updates", "skip-negative-range"),
                        ("lens_ignored", "lens-ok-0"), ("edge_falls_to_ok", "edge"), ("z_as_range", "ok-00-level0"), ("pose_swapped", "ok-00-level0"),
                        ("tau_no_quad", "ok-00-level0"), ("tau_quad_of_range", "ok-03-level1"), ("x_is_inverse_z", "ok-03-level1")):
        assert _changed(mc.by_name(name), fault), (fault, name)
    assert dm.restate(**mc.inputs(mc.by_name("ok-no-parallax")), fault="parallax_kept")["outcome"] == SKIPPED


def test_lookup_is_depth_seeds_rule_at_whole_pixels():
    """at whole-numbered level-0 positions the lookup is depth_seed's, status by status and sample by sample, with and without a lens"""
    rng = np.random.default_rng(20261101)
    for kind, scale in (("f32", 1.0), ("u16", mc.U16_SCALE), ("few", 1.0), ("edge", 1.0), ("hole", 1.0)):
        d = mc.image(kind)
        for dist in (None, mc.LENS, mc.LENS_OUT):
            for level in range(5):
                s = 1 << level
                xy = np.stack([rng.integers(0, mc.W // s + 1, 12), rng.integers(0, mc.H // s + 1, 12)], 1)
                xyl = np.concatenate([xy, np.full((12, 1), level)], 1)
                cam4 = (mc.CAM["fx"], mc.CAM["fy"], mc.CAM["u0"], mc.CAM["v0"])
                z, status, _ = dsr.depth_seed(d, xyl, cam4, dist, scale)
                for i in range(12):
                    got = dm.lookup(d, (float(xy[i, 0] * s), float(xy[i, 1] * s)), level, mc.CAM, dist, scale)
                    assert got == (status[i], z[i]), (kind, dist, level, xy[i], got, status[i], z[i])


def test_centre_rounds_half_up():
    assert dm.centre((5.5, 3.5), mc.CAM) == (6.0, 4.0) and dm.centre((5.49, 3.49), mc.CAM) == (5.0, 3.0)
    assert dm.centre((-0.5, -0.51), mc.CAM) == (0.0, -1.0)
    fu, fv = dm.centre((math.nan, math.inf), mc.CAM)
    assert fu != fu and fv != fv


def test_noise_defaults():
    assert dm.noise() == dm.NOISE_DEFAULTS and dm.noise(0.01, 0.0) == dict(noise_abs=0.01, noise_quad=0.0015)


def test_tolerance_of_a_measured_update():
    """only exp is left: the bound is the floor plus MARGIN times what +-N_ULP on exp's result moves; the position of a fixed point keeps the
    floor alone"""
    for c in CASES:
        base, bound = mc.expected(c)
        if base["status"] != dsr.OK:
            continue
        for k, v in dr._numbers(base).items():
            floor = dr.FLOOR_ULP * math.ulp(v)
            assert bound[k] >= floor
            if base["outcome"] == SKIPPED or (c["state"]["fixed"] and k.startswith(("position", "row.P"))):
                assert bound[k] == floor, (c["name"], k)
        # moving the four calls a measured update does not make changes nothing
        assert repr(dm.restate(**dict(mc.inputs(c), ulps=(4, -4, 4, -4, 0)))) == repr(base)
