"""The sparse stereo rule's restatement (tests/stereo_restatement.py, the specification of sdvl_stereo_depth) on designed pairs whose
answer is known without it, every refusal, and `shelf` pairs against the renderer's true depth.  No GPU.

Measured on the oracle's filtered corners of `shelf` frames 0, 13, 26, 39, baseline 0.11 m, default rule (the caps stand beside them):
  frame   corners   OK share (>= 60 %)   median |disparity error| (<= 0.1 px)   OK corners off by > 1 px (<= 2 %)
      0       261        88.5 %                       0.036 px                              0.00 %   (> 0.5 px: 0.43 %)
     13       261        88.9 %                       0.067 px                              0.00 %   (> 0.5 px: 0.00 %)
     26       268        87.7 %                       0.063 px                              0.00 %   (> 0.5 px: 0.00 %)
     39       265        87.9 %                       0.072 px                              0.00 %   (> 0.5 px: 0.00 %)
Of the corners that are not OK, 21 - 30 a frame are NOMATCH, 2 - 7 EDGE, at most 1 AMBIGUOUS, none OUTSIDE.

Two hand cases of the rule as it is written come out differently from what one might expect of their names, and are asserted as the
rule gives them:
  * a constant pair is never OK, but its status is NOMATCH, not AMBIGUOUS: all costs are equal, ties go to the smallest disparity, so the
    argmin is the first of the range, an end, and NOMATCH is tested before AMBIGUOUS (whose test 100 S0 > uniqueness S2 is false anyway
    when both are 0).  AMBIGUOUS is shown on a periodic texture instead;
  * an integer shift recovers d with delta exactly 0 where S(d - 1) = S(d + 1) (the ramp); on a general texture S(d) = 0, d0 = d, and
    delta is whatever the two neighbours' costs make it, below half a pixel."""
import numpy as np
import pytest

import oraclelib as ol
import stereo_cases as stc
import stereo_restatement as sr


@pytest.fixture(scope="module")
def orc():
    return ol.Oracle()


def fb(c):
    return np.float64(c["cam"][0]) * np.float64(c["baseline"])


def test_integer_shift_is_exact():
    c = stc.designed_cases()["integer"]
    out = stc.restate(c)
    assert len(c["xyl"]) > 100 and set(c["xyl"][:, 2]) == {0, 1, 2}
    assert np.all(out["status"] == sr.OK) and np.all(out["d0"] == 7) and np.all(out["s0"] == 0)
    assert np.all(out["disparity"] == 7.0) and np.all(out["z"] == fb(c) / 7.0)
    assert np.array_equal(sr.d0_of(out["disparity"]), out["d0"])


def test_integer_shift_of_noise():
    c = stc.designed_cases()["noise"]
    out = stc.restate(c)
    assert set(c["xyl"][:, 2]) == {0, 1, 2, 3}
    assert np.all(out["status"] == sr.OK) and np.all(out["d0"] == 11) and np.all(out["s0"] == 0)
    assert np.all(np.abs(out["disparity"] - 11.0) < 0.5)
    assert np.array_equal(sr.d0_of(out["disparity"]), out["d0"])


def test_half_pixel_shift():
    """a steep ramp between two integer shifts: the cost is a V about d + 0.5 with S(d) = S(d + 1) = 162 and S(d - 1) = S(d + 2) = 486.
    Stated: OK, the tie goes to d0 = d = 9, delta = +0.5 exactly (|delta| <= 0.5 with equality), the disparity 9.5"""
    c = stc.designed_cases()["half"]
    out = stc.restate(c)
    assert len(c["xyl"]) >= 100
    assert np.all(out["status"] == sr.OK) and np.all(out["d0"] == 9) and np.all(out["s0"] == 162)
    assert np.all(out["disparity"] - out["d0"] == 0.5) and np.all(out["z"] == fb(c) / 9.5)
    assert np.array_equal(sr.d0_of(out["disparity"]), out["d0"])


def test_constant_pair_is_never_ok():
    for name in ("constant", "constant1"):
        c = stc.designed_cases()[name]
        out = stc.restate(c)
        assert np.all(out["status"] != sr.OK)
        assert np.array_equal(out["status"], c["want"]) and np.all(out["d0"] == 0)      # the tie rule: the first disparity of the range
        assert np.all(out["z"] == 0.0) and np.all(out["disparity"] == 0.0)


def test_periodic_texture_is_ambiguous():
    c = stc.designed_cases()["periodic"]
    out = stc.restate(c)
    assert np.array_equal(out["status"], c["want"]), out["status"]
    assert np.all(out["d0"] == 2) and np.all(out["s0"] == 81)      # the smallest of the equal minima 2, 10, 18, ...
    # with a uniqueness that asks for nothing, the same corners pass
    assert np.all(sr.stereo_depth(c["left"], c["right"], c["xyl"], c["cam"], c["baseline"], uniqueness=100)["status"] == sr.OK)


def test_outside():
    c, want = stc.outside_case()
    out = stc.restate(c)
    assert len(want) == len(c["xyl"])
    for i, w in enumerate(want):
        if w is None:
            assert out["status"][i] != sr.OUTSIDE, (i, c["xyl"][i])
        else:
            assert out["status"][i] == w, (i, c["xyl"][i], out["status"][i])
    assert (out["status"] == sr.OUTSIDE).sum() >= 30 and (out["status"] != sr.OUTSIDE).sum() >= 9


@pytest.mark.parametrize("k", [0, 1, 2])
def test_best_at_a_range_end_is_nomatch(k):
    c = stc.range_end_case()[k]
    out = stc.restate(c)
    assert np.array_equal(out["status"], c["want"])
    assert np.all(out["d0"] == (7, 0, 9)[k]) and np.all(out["s0"] == 0)


def test_max_depth_starts_the_range_above_zero():
    hit, miss = stc.d_lo_case()
    out = stc.restate(hit)
    assert np.all(out["status"] == sr.OK) and np.all(out["disparity"] == 12.0)
    out = stc.restate(miss)
    assert np.all(out["status"] == sr.NOMATCH) and np.all(out["d0"] == 5)


def test_window_on_two_depths_is_edge():
    c = stc.designed_cases()["edge"]
    out = stc.restate(c)
    assert np.array_equal(out["status"], c["want"]), out["status"]
    assert np.all(out["d0"][:3] == 7) and np.all(out["disparity"][3:] == 5.0)
    # the four half windows of the straddling corner: columns 0-4 on the near surface alone, the others a compromise
    cst = sr.costs(c["left"], c["right"], stc.EDGE_X, 60, 1, 0, 40)
    assert [int(np.argmin(cst[k])) for k in range(5)][:2] == [7, 5]


@pytest.mark.parametrize("n_range", stc.RANGES)
def test_range_cases_search_what_they_say(n_range):
    """the pairs the device test uses around the lane rounds: the corners past the range's own limit search exactly n_range disparities
    and, where the shift lies inside the range, find it"""
    c = stc.range_case(n_range)
    r = sr.rule(c["baseline"], **c["rule"])
    _, d_lo, d_cap = sr.call_range(c["cam"][0], r)
    assert (d_lo, d_cap) == (0, max(n_range - 1, 1))
    xyl = c["xyl"].astype(np.int64)
    s = 1 << xyl[:, 2]
    full = xyl[:, 0] * s - 4 * s >= d_cap
    assert full.sum() >= 12 and set(xyl[full, 2]) == {0, 1, 2, 3} and (~full).sum() >= 1
    out = stc.restate(c)
    if n_range > 3:
        ok = out["status"] == sr.OK
        assert ok[full].sum() >= full.sum() // 2, np.bincount(out["status"], minlength=5)
        assert np.all(np.abs(out["disparity"][ok] - (2 * n_range) // 3) < 0.5)


def test_defaults_and_zero_fields():
    assert sr.rule(0.1) == dict(sr.DEFAULTS, baseline=0.1)
    assert sr.rule(0.1, max_sad=0, uniqueness=0, min_depth=0.0) == dict(sr.DEFAULTS, baseline=0.1)
    assert sr.rule(0.1, max_disparity=511)["max_disparity"] == 511
    fb_, d_lo, d_cap = sr.call_range(517.3, sr.rule(0.11))
    assert (d_lo, d_cap) == (0, int(np.floor(517.3 * 0.11 / 0.3)))
    assert sr.call_range(517.3, sr.rule(0.11, min_depth=0.01))[2] == 192      # the cap is max_disparity


def test_refusals():
    left = stc.ramp()
    right = stc.shifted(left, 3)
    xyl = [(80, 60, 0)]
    good = dict(left=left, right=right, xyl=xyl, cam=ol.TUM_CAM, baseline=0.11)

    def refused(**kw):
        a = dict(good)
        rule = {k: kw.pop(k) for k in list(kw) if k in sr.DEFAULTS}
        a.update(kw)
        with pytest.raises(sr.Refused):
            sr.stereo_depth(a.pop("left"), a.pop("right"), a.pop("xyl"), a.pop("cam"), a.pop("baseline"), **a, **rule)

    for b in (0.0, -0.1, float("nan"), float("inf")):
        refused(baseline=b)
    refused(max_disparity=512)
    refused(max_disparity=-1)
    refused(uniqueness=101)
    refused(uniqueness=-1)
    refused(max_sad=256)
    refused(max_sad=-1)
    refused(min_depth=-0.1)
    refused(xyl=[(10, 10, 5)])                      # a level outside a pyramid of five
    refused(xyl=[(10, 10, -1)])
    refused(dist=(0.1, 0, 0, 0, 0))                 # a lens
    refused(right=right[:, :-1])                    # (the device's form of this: a stride below the width)
    sr.stereo_depth(left, right, xyl, ol.TUM_CAM, 0.11, dist=(0.0, 0.2, 0, 0, 0))      # d[0] == 0: no lens
    # job ranges
    for jobs in ([(left, right, 0, 2)], [(left, right, -1, 1)], [(left, right, 1, 0)], [(left, right, 0, 1), (left, right, 0, 1)]):
        with pytest.raises(sr.Refused):
            sr.stereo_jobs(jobs, xyl, ol.TUM_CAM, 0.11)
    z, disp, status, ok = sr.stereo_jobs([(left, right, 0, 0)], xyl, ol.TUM_CAM, 0.11)
    assert list(status) == [sr.NOMATCH] and list(ok) == [0]      # a corner no job names


def test_track_sequence_help_and_refusals():
    """host/track_sequence names both stereo forms in --help and refuses the combinations that throw before any device is touched
    (exit status 2 with a message; a machine without a GPU would answer 1 at the first device call)"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--stereo --baseline B" in r.stdout and "--right-list FILE --baseline B" in r.stdout
    stereo = ["--synthetic", "2", "--scene", "shelf", "--stereo", "--baseline", "0.11"]
    for args, word in ((["--synthetic", "2", "--stereo", "--baseline", "0.11"], "--scene"),
                       (["--synthetic", "2", "--scene", "shelf", "--stereo"], "--baseline"),
                       (stereo[:-1] + ["0"], "--baseline"),
                       (stereo + ["--depth"], "--depth"),
                       (stereo + ["--init", "two-frame"], "two-frame"),
                       (stereo + ["--dist", "0.1", "0", "0", "0", "0"], "lens"),
                       (stereo + ["--batch"], "--batch"),
                       (stereo + ["--depth-mapping"], "--depth-mapping"),
                       (stereo + ["--depth-bundle"], "--depth-bundle"),
                       (["--synthetic", "2", "--right-list", "right.txt", "--baseline", "0.11"], "--list")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)


@pytest.mark.parametrize("k", stc.SHELF_FRAMES)
def test_shelf_against_the_true_depth(orc, k):
    c, depth = stc.shelf_pair(orc, k)
    out = stc.restate(c)
    ok = out["status"] == sr.OK
    err = np.abs(out["disparity"][ok] - stc.true_disparity(c, depth)[ok])
    counts = np.bincount(out["status"], minlength=5)
    print("shelf frame %d: %d corners, OK %d NOMATCH %d AMBIGUOUS %d EDGE %d OUTSIDE %d; OK share %.1f %%, median error %.4f px, off by > 1 px %.2f %%, "
          "off by > 0.5 px %.2f %%" % (k, len(ok), counts[0], counts[1], counts[2], counts[3], counts[4], 100 * ok.mean(), np.median(err),
                                     100 * (err > 1.0).mean(), 100 * (err > 0.5).mean()))
    assert np.median(err) <= 0.1
    assert (err > 1.0).mean() <= 0.02
    assert ok.mean() >= 0.60
    assert np.all(out["z"][~ok] == 0.0) and np.all(out["disparity"][~ok] == 0.0)
    assert np.array_equal(sr.d0_of(out["disparity"][ok]), out["d0"][ok])
