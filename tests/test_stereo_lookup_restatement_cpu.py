"""The stereo lookup's restatement and the depth filter fed by it (tests/stereo_lookup_restatement.py, the specification of
sdvl_stereo_lookup, sdvl_depth_filter_stereo and sdvl_search_run_filter_stereo) on the cases of tests/stereo_lookup_cases.py; the refusals;
host/track_sequence's flags; host/stereo_map_check's half that needs no device.  No GPU.

Measured on the oracle's filtered corners of `shelf` frames 0, 13, 26, 39, displaced below the stride (stereo_lookup_cases.shelf_jittered),
baseline 0.11 m, default rule, against the renderer's true disparity at the rounded centre (the caps stand beside them):
  frame   positions   OK share (>= 60 %)   median |disparity error| (<= 0.1 px)   OK positions off by > 1 px (<= 2 %)
      0        261         87.7 %                       0.029 px                              0.00 %
     13        261         89.7 %                       0.073 px                              0.00 %
     26        268         87.3 %                       0.062 px                              0.00 %
     39        265         88.3 %                       0.070 px                              0.00 %
"""
import os
import subprocess

import numpy as np
import pytest

import depth_measure_cases as dmc
import depth_measure_restatement as dmr
import depth_restatement as dr
import depth_seed_restatement as dsr
import oraclelib as ol
import stereo_cases as stc
import stereo_lookup_cases as slc
import stereo_lookup_restatement as sl
import stereo_restatement as sr
from depth_restatement import CONVERGED, UPDATED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc():
    return ol.Oracle()


def same_bits(got, want):
    z, disp, status, _ = got
    return (np.array_equal(status, want["status"]) and z.tobytes() == want["z"].tobytes() and disp.tobytes() == want["disparity"].tobytes())


# ---------------------------------------------------------------------------------------------------- the lookup
@pytest.mark.parametrize("name", sorted(stc.designed_cases()))
def test_identity_on_the_designed_cases(name):
    """a level-l corner looked up within half a pixel of (x s, y s): sdvl_stereo_depth's restatement, bit for bit"""
    c = stc.designed_cases()[name]
    px, lv = slc.positions_of(c)
    assert np.abs(px - np.round(px)).max() < 0.5 and (np.abs(px - np.round(px)) > 0.4).any()
    got = sl.stereo_lookup([(c["left"], c["right"], 0, len(px))], px, lv, c["cam"], c["baseline"], **c["rule"])
    assert same_bits(got, stc.restate(c)), name


@pytest.mark.parametrize("k", stc.SHELF_FRAMES[:2])
def test_identity_on_shelf(orc, k):
    c, _ = stc.shelf_pair(orc, k)
    px, lv = slc.positions_of(c)
    got = sl.stereo_lookup([(c["left"], c["right"], 0, len(px))], px, lv, c["cam"], c["baseline"])
    want = stc.restate(c)
    assert same_bits(got, want) and (want["status"] == sr.OK).sum() >= 150


def test_centre_rule():
    c, px, lv, want = slc.centre_cases()
    z, disp, status, ok = sl.stereo_lookup([(c["left"], c["right"], 0, len(px))], px, lv, c["cam"], c["baseline"])
    fb = np.float64(c["cam"][0]) * np.float64(c["baseline"])
    seen = set()
    for i, w in enumerate(want):
        if w is None:
            assert status[i] != sr.OUTSIDE, (i, px[i], lv[i])
        elif isinstance(w, tuple):
            ref = sr.stereo_depth(c["left"], c["right"], [w[1:]], c["cam"], c["baseline"])
            assert (status[i], disp[i], z[i]) == (ref["status"][0], ref["disparity"][0], ref["z"][0]) and status[i] == sr.OK, (i, px[i], w)
        else:
            assert status[i] == w, (i, px[i], lv[i], status[i], w)
            if w == sr.OK:
                assert disp[i] == 7.0 and z[i] == fb / 7.0, (i, px[i], disp[i])
        seen.add(int(status[i]))
    assert {sr.OK, sr.OUTSIDE} <= seen and int(ok[0]) == int((status == sr.OK).sum())
    # level 2 with an odd centre is no corner of that level
    odd = [i for i in range(len(px)) if lv[i] == 2 and int(np.floor(px[i][0] + 0.5)) % 2 == 1 and status[i] == sr.OK]
    assert len(odd) >= 4


def test_jobs_unnamed_positions_and_counts():
    a, b = stc.designed_cases()["noise"], stc.designed_cases()["integer"]
    pa, la = slc.positions_of(a)
    pb, lb = slc.positions_of(b)
    na, nb = 40, 30
    px = np.concatenate([pa[:na], pb[:2], pb[:nb], pa[:1]])
    lv = np.concatenate([la[:na], lb[:2], lb[:nb], la[:1]])
    jobs = [(a["left"], a["right"], 0, na), (b["left"], b["right"], na + 2, na + 2), (b["left"], b["right"], na + 2, na + 2 + nb)]
    z, disp, status, ok = sl.stereo_lookup(jobs, px, lv, ol.TUM_CAM, stc.BASELINE)
    assert list(status[na:na + 2]) == [sr.NOMATCH] * 2 and status[-1] == sr.NOMATCH and list(ok) == [na, 0, nb]
    assert np.all(z[na:na + 2] == 0.0) and z[-1] == 0.0
    z0, _, s0, ok0 = sl.stereo_lookup([], np.zeros((0, 2)), [], ol.TUM_CAM, stc.BASELINE)
    assert len(z0) == 0 and len(s0) == 0 and len(ok0) == 0


@pytest.mark.parametrize("k", stc.SHELF_FRAMES)
def test_shelf_at_jittered_positions(orc, k):
    """the caps of test_shelf_against_the_true_depth at positions off the corners and off the levels' grids"""
    c, depth, px, lv, centres = slc.shelf_jittered(orc, k)
    s = 1 << lv.astype(np.int64)
    assert ((centres[:, 0] % s != 0) & (lv > 0)).sum() >= 20          # centres that are no multiple of their stride
    z, disp, status, _ = sl.stereo_lookup([(c["left"], c["right"], 0, len(px))], px, lv, c["cam"], c["baseline"])
    ok = status == sr.OK
    err = np.abs(disp[ok] - slc.true_disparity_at(c, depth, centres)[ok])
    counts = np.bincount(status, minlength=5)
    print("shelf frame %d: %d positions, OK %d NOMATCH %d AMBIGUOUS %d EDGE %d OUTSIDE %d; OK share %.1f %%, median error %.4f px, off by > 1 px %.2f %%"
          % (k, len(ok), counts[0], counts[1], counts[2], counts[3], counts[4], 100 * ok.mean(), np.median(err), 100 * (err > 1.0).mean()))
    assert np.median(err) <= 0.1
    assert (err > 1.0).mean() <= 0.02
    assert ok.mean() >= 0.60
    assert np.all(z[~ok] == 0.0) and np.all(disp[~ok] == 0.0)


# ---------------------------------------------------------------------------------------------------- the filter
CASES = slc.all_cases()


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_filter_case(name):
    c = slc.by_name(name)
    base = slc.check(c)
    tri = dr.restate(**slc.triangulated_inputs(c))
    if base["status"] != sr.OK:
        # a miss, a hit in no job, every status that is not OK: depth_restatement's bits
        for k in ("outcome", "n_failed", "rho", "sigma2", "a", "b", "cos_alpha", "last_distance", "position", "row"):
            assert base[k] == tri[k], (name, k)
        assert base["disparity"] == 0.0
    else:
        status, disp, zc = slc.matched(c["pair"], c["px"], c["level"], c["rule"])
        assert status == sr.OK and base["disparity"] == disp
        fb = float(np.float64(c["cam"]["fx"]) * np.float64(c["baseline"]))
        sigma = c["disparity_sigma"] if c["disparity_sigma"] != 0 else 0.25
        if "tau" in base["trace"]:
            assert base["trace"]["z"] == zc and base["trace"]["tau"] == (sigma / fb) * (zc * zc)
            assert abs(base["trace"]["tau"] - sigma * zc * zc / fb) <= 4 * np.spacing(base["trace"]["tau"])
        if c["want"].get("exact_range") and base["outcome"] in (UPDATED, CONVERGED):
            assert abs(base["trace"]["depth"] - c["range"]) <= 1e-9 * c["range"]
            r0, r1, truth = c["state"]["rho"], base["rho"], 1.0 / c["range"]
            assert min(r0, truth) - 1e-12 <= r1 <= max(r0, truth) + 1e-12


def test_the_cases_cover_every_status_and_outcome():
    seen = {(sl.restate(**slc.inputs(c))["status"]) for c in CASES}
    assert seen == {sr.OK, sr.NOMATCH, sr.AMBIGUOUS, sr.EDGE, sr.OUTSIDE, sl.NO_LOOKUP}
    assert len(slc.groups()["plain"]) >= 20


@pytest.mark.parametrize("fault", sorted(sl.FAULTS))
def test_every_planted_fault_is_caught(fault):
    """at least one case's result leaves its bound, or changes its status or outcome, when the error is planted"""
    caught = []
    cases = list(CASES)
    if fault in ("centre_truncated", "centre_on_grid", "stride_level0", "range_of_grid"):
        cases = cases + _lookup_fault_cases()
    for c in cases:
        if "lookup_only" in c:
            good, bad = sl.lookup(*c["lookup_only"]), sl.lookup(*c["lookup_only"], fault=fault)
            if good != bad:
                caught.append(c["name"])
            continue
        bad = sl.restate(**dict(slc.inputs(c), fault=fault))
        d, _ = slc.differences(c, bad)
        if d:
            caught.append(c["name"])
    print("%s: caught by %s" % (fault, caught))
    assert caught, (fault, sl.FAULTS[fault])


def _lookup_fault_cases():
    """positions whose answer depends on the centre and the stride being the rule's: on a `shelf`-free pair, noise shifted by 11"""
    c = stc.designed_cases()["noise"]
    left, right = np.asarray(c["left"]), np.asarray(c["right"])
    out = []
    for i, (px, l) in enumerate((((90.7, 60.6), 0), ((91.2, 61.3), 2), ((93.4, 57.2), 3), ((47.3, 60.2), 3), ((45.6, 33.3), 2))):
        out.append(dict(name="lookup-%d" % i, lookup_only=(left, right, px, l, ol.TUM_CAM, stc.BASELINE)))
    return out


def test_measured_update_equals_depth_measure_restatement():
    """the measured update restated here for a general (noise_abs, noise_quad), against depth_measure_restatement.restate on its own cases
    with constant depth images and non-zero noise: the copy stays tied to the original, bit for bit"""
    n = 0
    for c in dmc.all_cases():
        if not c["found"] or c["depth"] is None or c["dist"] is not None:
            continue
        for zc, (na, nq) in ((1.5, (0.004, 0.002)), (1.25, (0.001, 0.0015)), (2.0, (1e-6, 0.3))):
            img = np.full(c["depth"].shape, zc, np.float32)
            kw = dict(dmc.inputs(c), depth=img, scale=1.0, rule={}, noise_abs=na, noise_quad=nq)
            want = dmr.restate(**kw)
            if want["status"] != dsr.OK:
                continue
            got = sl.measured_update(c["cur_pose"], c["ref_pose"], c["bearing"], c["px"], c["cam"], c["state"], c["params"], float(np.float32(zc)), na, nq)
            for k in ("outcome", "n_failed", "rho", "sigma2", "a", "b", "cos_alpha", "last_distance", "position", "row", "trace"):
                assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (c["name"], zc, k, got[k], want[k])
            n += 1
            for fault in ("z_as_range", "pose_swapped", "parallax_kept", "no_depth_mean_test", "negative_depth_updates", "x_is_inverse_z"):
                a = sl.measured_update(c["cur_pose"], c["ref_pose"], c["bearing"], c["px"], c["cam"], c["state"], c["params"], float(np.float32(zc)), na, nq, fault)
                b = dmr.restate(**dict(kw, fault=fault))
                assert all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in ("outcome", "rho", "sigma2", "a", "b", "position")), (c["name"], fault)
    assert n >= 40


def test_stereo_noise():
    cam = slc.CAM
    fb = float(np.float64(cam["fx"]) * np.float64(0.11))
    assert sl.stereo_noise(cam, 0.11, 0.4) == (0.0, 0.4 / fb)
    assert sl.stereo_noise(cam, 0.11, 0.0) == (0.0, 0.25 / fb) and sl.DISPARITY_SIGMA == 0.25
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(sl.Refused):
            sl.stereo_noise(cam, 0.11, bad)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    left = stc.ramp()
    right = stc.shifted(left, 3)
    px, lv = [(80.2, 60.3)], [0]

    def refused(jobs=None, px_=px, lv_=lv, **kw):
        with pytest.raises(sr.Refused):
            sl.stereo_lookup(jobs if jobs is not None else [(left, right, 0, 1)], px_, lv_, ol.TUM_CAM, kw.pop("baseline", 0.11), **kw)

    for b in (0.0, -0.1, float("nan"), float("inf")):
        refused(baseline=b)
    refused(max_disparity=512)
    refused(max_disparity=-1)
    refused(uniqueness=101)
    refused(uniqueness=-1)
    refused(max_sad=256)
    refused(max_sad=-1)
    refused(min_depth=-0.1)
    refused(lv_=[5])                                # a level outside a pyramid of five
    refused(lv_=[-1])
    refused(lv_=[0, 0])                             # one level per position
    refused(dist=(0.1, 0, 0, 0, 0))                 # a lens
    refused(jobs=[(left, right[:, :-1], 0, 1)])
    for jobs in ([(left, right, 0, 2)], [(left, right, -1, 1)], [(left, right, 1, 0)], [(left, right, 0, 1), (left, right, 0, 1)]):
        refused(jobs=jobs)
    sl.stereo_lookup([(left, right, 0, 1)], px, lv, ol.TUM_CAM, 0.11, dist=(0.0, 0.2, 0, 0, 0))      # d[0] == 0: no lens
    z, disp, status, ok = sl.stereo_lookup([(left, right, 0, 0)], px, [7], ol.TUM_CAM, 0.11)        # a position no job names: its level is not looked at
    assert list(status) == [sr.NOMATCH] and list(ok) == [0]


def test_track_sequence_help_and_refusals():
    """host/track_sequence names the switch in --help and refuses what cannot go with it before any device is touched"""
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--stereo-mapping [--disparity-sigma X]" in r.stdout and "not measured against a real pair" in r.stdout
    stereo = ["--synthetic", "2", "--scene", "shelf", "--stereo", "--baseline", "0.11"]
    for args, word in ((["--synthetic", "2", "--scene", "shelf", "--stereo-mapping"], "--stereo"),
                       (["--synthetic", "2", "--scene", "shelf", "--depth", "--stereo-mapping"], "--stereo"),
                       (stereo + ["--stereo-mapping", "--disparity-sigma", "-0.5"], "--disparity-sigma"),
                       (stereo + ["--stereo-mapping", "--disparity-sigma", "nan"], "--disparity-sigma"),
                       (stereo + ["--disparity-sigma", "0.3"], "--stereo-mapping"),
                       (stereo + ["--stereo-mapping", "--disparity-sigma"], "missing value"),
                       (stereo + ["--stereo-mapping", "--depth-mapping"], "--depth-mapping"),
                       (stereo + ["--stereo-mapping", "--batch"], "--batch"),
                       (stereo + ["--stereo-mapping", "--init", "two-frame"], "two-frame")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)


def test_host_check():
    """host/stereo_map_check without --device: the rules of MapperMap::SetStereoMapping that need no device"""
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "stereo_map_check")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "(mapper): 0 failed" in r.stdout, r.stdout + r.stderr
