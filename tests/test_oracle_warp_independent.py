"""Matcher::WarpMatrixAffine, GetSearchLevel and CreatePatch (matcher.cc:293-357) under warps far from the identity: the ORACLE
against a float64 numpy restatement written from the reference's text, and against the renderer's own geometry.

Every other test renders its two views a few frames apart, where A^-1 is 2^-level times a near-identity: swapped off-diagonal
terms, a transposed A, a mishandled negative entry or a wrong out-of-image test would pass there.  Here the current view is rolled
30 and 90 degrees, tilted 25 degrees with a sideways baseline, zoomed 1.9x with a 20 degree roll, and zoomed out to 0.6x.

Search levels the views reach (a property of det A ~ zoom^2 * 4^level, checked below): roll and tilt 0, 1, 2; zoom 1.9 only 1, 2
(3.61 > 3 already at level 0); zoom 0.6 only 0, 1 (0.36 * 16 = 5.76 < 12)."""
import numpy as np
import pytest

from oraclelib import WARP_CAM, WARP_VIEWS, warp_border_case, warp_view_case
from warp_restatement import create_patch, relative_pose, restate_border_case, search_level, warp_matrix

MODES = [True, False]
CASES = [(v, f) for v in WARP_VIEWS for f in MODES]
IDS = ["%s-%s" % (v, "fixed" if f else "epipolar") for v, f in CASES]


def bilinear(im, x, y):
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    ax, ay = x - x0, y - y0
    return (1 - ax) * (1 - ay) * im[y0, x0] + (1 - ax) * ay * im[y0 + 1, x0] + ax * (1 - ay) * im[y0, x0 + 1] + ax * ay * im[y0 + 1, x0 + 1]


@pytest.fixture(scope="module")
def restated(orc, synth):
    """per case: the restatement's A, search level and patch for each of its requests"""
    memo = {}

    def get(view, fixed):
        if (view, fixed) not in memo:
            c = warp_view_case(orc, synth, view, fixed)
            pyr = orc.pyramid(c["img_ref"], 5)
            R, t = relative_pose(c["T_ref"], c["T_cur"])
            out = []
            for m in c["meta"]:
                A = warp_matrix(R, t, m["px"], m["bearing"], 1.0 / m["idepth"], m["level"])
                sl = search_level(A)
                patch, outside = create_patch(np.linalg.inv(A), pyr[m["level"]], m["px"], m["level"], sl)
                out.append(dict(A=A, slevel=sl, patch=patch, outside=outside))
            memo[(view, fixed)] = out
        return memo[(view, fixed)]
    return get


def check_inputs(c, view):
    """conditions on the INPUTS, judged on the oracle alone: the case has not gone empty and reaches the search levels it can"""
    want = c["want"]
    assert len(want) == 120
    assert sum(w["found"] for w in want) >= c["found_floor"], (sum(w["found"] for w in want), c["found_floor"])
    assert all(w["stage"] >= 1 for w in want)       # every request passes the projection and margin tests: every one has a patch
    levels = {w["slevel"] for w in want}
    assert levels == ({1, 2} if view.startswith("zoom1.9") else {0, 1} if view.startswith("zoom0.6") else {0, 1, 2}), levels


@pytest.mark.parametrize("view,fixed", CASES, ids=IDS)
def test_search_level_equals_the_restatement(orc, synth, restated, view, fixed):
    """GetSearchLevel of the oracle's A = the restatement's, for every request.  A request whose determinant sits within 1e-9
    relative of a threshold of the loop (3, 12; 48 for a deeper loop) may fall either way and is skipped — at most 2 % of a view.
    Measured: none is skipped in any of the ten cases."""
    c = warp_view_case(orc, synth, view, fixed)
    check_inputs(c, view)
    skipped = 0
    for w, r in zip(c["want"], restated(view, fixed)):
        det = np.linalg.det(r["A"])
        if any(abs(det - thr) <= 1e-9 * thr for thr in (3.0, 12.0, 48.0)):
            skipped += 1
            continue
        assert w["slevel"] == r["slevel"], (det, w["slevel"], r["slevel"])
    print("%s: %d of %d requests skipped at a level threshold" % (view, skipped, len(c["want"])))
    assert skipped <= 0.02 * len(c["want"])


@pytest.mark.parametrize("view,fixed", CASES, ids=IDS)
def test_border_patch_equals_the_restatement_within_one_grey_level(orc, synth, restated, view, fixed):
    """The oracle's 10x10 border patch against the restated one: the oracle interpolates in float32, the restatement in float64,
    so the truncation to 8 bits may land on either side of an integer — one grey level, never two.  Pixels that differ at all,
    measured (fixed = epipolar, the patch does not depend on the mode): roll 30 0.117 %, roll 90 10.992 %, tilt 25 0.008 %, zoom 1.9 + roll 20 0.017 %,
    zoom 0.6 12.158 % of the 12000 pixels of a case.  The two large shares are exact ties, not error: at roll 90 the samples sit within
    1e-14 of integer coordinates (I00 ~ 6e-17), where the float32 coordinate is the integer itself and the float64 one may lie just
    below it; at zoom 0.6 the level-0 samples are thirds of a pixel, where the interpolated value is often an integer up to rounding.
    Asserted: below 50 %, so that a patch that is shifted as a whole cannot hide inside the +-1.  No patch of these requests leaves the reference image, not even at zoom 0.6 (detected corners
    keep 19 pixels from the border of their level, the widest grid here reaches 8.4): the out-of-image rule has its own test below."""
    c = warp_view_case(orc, synth, view, fixed)
    check_inputs(c, view)
    differ = total = zeroed = 0
    for i, (w, r) in enumerate(zip(c["want"], restated(view, fixed))):
        got = w["border"].reshape(10, 10).astype(np.int32)
        d = np.abs(got - r["patch"].astype(np.int32))
        assert d.max() <= 1, (i, int(d.max()), r["A"])
        assert np.all(got[r["outside"]] == 0)
        differ += int(np.count_nonzero(d)); total += d.size; zeroed += int(r["outside"].sum())
    print("%s %s: %.3f %% of %d patch pixels differ by one grey level; %d samples outside the image"
          % (view, "fixed" if fixed else "epipolar", 100.0 * differ / total, total, zeroed))
    assert differ < 0.5 * total


@pytest.mark.parametrize("view", ["roll30", "zoom0.6"])
def test_out_of_image_rule_on_patches_that_leave_the_reference_image(orc, synth, view):
    """Requests that are no corners (oraclelib.warp_border_case): points 6 to 9 pixels (of their level) inside each border of the
    reference image.  Rolled by 30 degrees or spread by 1 / 0.6 their sample grids cross the border: samples outside are zero, the
    same samples in the oracle and in the restatement, every other sample within one grey level.  Measured: 60 samples of 37
    requests outside at roll 30, 511 of 34 at zoom 0.6, of 18000."""
    c = warp_border_case(orc, synth, view)
    restated = restate_border_case(orc, c)
    zeroed = sum(int(r["outside"].sum()) for r in restated)
    assert zeroed >= 40 and 100 * len(restated) - zeroed >= 10 * zeroed, zeroed      # the inputs do cross the border, and only just
    for m, w, r in zip(c["meta"], c["want"], restated):
        assert w["stage"] >= 1, (m["level"], m["px"])           # past the margin test: the patch was made
        assert w["slevel"] == r["slevel"]
        got = w["border"].reshape(10, 10).astype(np.int32)
        assert np.all(got[r["outside"]] == 0), (m["level"], m["px"])
        assert np.abs(got - r["patch"].astype(np.int32)).max() <= 1, (m["level"], m["px"])
    print("%s: %d samples of %d requests outside the reference image, of %d" % (
        view, sum(int(r["outside"].sum()) for r in restated), sum(bool(r["outside"].any()) for r in restated), 100 * len(restated)))


@pytest.mark.parametrize("view", ["roll30", "roll90"])
def test_rolled_patch_looks_like_the_current_image_where_the_homography_puts_it(orc, synth, view):
    """No restatement here.  For a roll by theta about the optical axis the plane-induced homography is the rotation of the pixel
    plane about the principal point, px_cur = c + Rot(theta) (px - c), and the warped patch is the current image's own 10x10
    neighbourhood of px_cur on the search level.  Mean absolute grey-level difference between the two over the requests whose
    patches are interior, against the same figure for the patch of A = 2^level * Identity (the unrotated neighbourhood of the
    reference corner): the warped patch must be closer by a factor of at least 2 — loose on purpose, it is there to catch a
    transposed or sign-flipped warp (which rotates the patch the other way and is no better than the identity), not rounding.
    Measured: factor 11.83 at roll 30 (mean |difference| 2.18 against 25.78, 109 interior patches), 16.27 at roll 90 (2.48 against 40.35, 90 patches)."""
    c = warp_view_case(orc, synth, view, True)
    check_inputs(c, view)
    theta = WARP_VIEWS[view][0][5]
    rot = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    pyr_ref, pyr_cur = orc.pyramid(c["img_ref"], 5), orc.pyramid(c["img_cur"], 5)
    centre = WARP_CAM[2:]
    gx, gy = np.meshgrid(np.arange(10) - 5.0, np.arange(10) - 5.0)
    mad_warp, mad_ident, n = 0.0, 0.0, 0
    for m, w in zip(c["meta"], c["want"]):
        sl, l = w["slevel"], m["level"]
        assert sl == l                                             # a rotation has det A = 4^level
        pc = (centre + rot @ (m["px"] - centre)) / (1 << sl)
        cur = pyr_cur[sl].astype(np.float64)
        if pc[0] - 5 < 0 or pc[1] - 5 < 0 or pc[0] + 5 >= cur.shape[1] - 1 or pc[1] + 5 >= cur.shape[0] - 1:
            continue                                               # the neighbourhood in the current image is not interior
        x, y = int(m["px"][0]) >> l, int(m["px"][1]) >> l
        ref = pyr_ref[l]
        if x - 8 < 0 or y - 8 < 0 or x + 8 >= ref.shape[1] - 1 or y + 8 >= ref.shape[0] - 1:
            continue                                               # the rotated 10x10 grid (half diagonal 7.1) could leave the reference
        there = bilinear(cur, pc[0] + gx, pc[1] + gy)
        mad_warp += np.abs(w["border"].reshape(10, 10) - there).mean()
        mad_ident += np.abs(ref[y - 5:y + 5, x - 5:x + 5] - there).mean()
        n += 1
    assert n >= 30, n
    print("%s: %d interior patches, mean |warped - current| = %.2f, mean |identity - current| = %.2f, factor %.2f"
          % (view, n, mad_warp / n, mad_ident / n, mad_ident / mad_warp))
    assert mad_warp * 2.0 <= mad_ident
