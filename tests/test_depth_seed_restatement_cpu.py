"""The depth-seeding rule's restatement (tests/depth_seed_restatement.py, the specification of sdvl_depth_seed) on designed inputs whose
answer is known without it: a plane, a depth step of 1 % and of 20 %, holes, too few samples, windows that leave a small image, the
depth limits, the `shelf` scene through a lens against the analytic depth of every corner's ray, and the counts on six `shelf` frames.
No GPU."""
import numpy as np
import pytest

import depth_seed_cases as dc
import depth_seed_restatement as dr
import oraclelib as ol


@pytest.fixture(scope="module")
def orc():
    return ol.Oracle()


@pytest.mark.parametrize("name", ["plane", "holes", "few6", "few5", "border", "range"])
def test_designed_statuses(name):
    c = dc.designed_cases()[name]
    z, status, _ = dc.restate(c)
    assert np.array_equal(status, c["want"]), (name, status, c["want"])
    ok = status == dr.OK
    assert np.all(z[~ok] == 0.0)
    # the depth is the centre sample itself, converted once
    fu, fv = dr.centre_pixels(c["xyl"], c["cam"], c["dist"])
    for i in np.flatnonzero(ok):
        assert z[i] == np.float64(c["depth"][int(fv[i]), int(fu[i])])


def test_plane_depth_is_exact():
    z, status, rel = dc.restate(dc.designed_cases()["plane"])
    assert np.all(status == dr.OK) and np.all(z == 1.5) and np.all(rel == 0.0)


@pytest.mark.parametrize("height,edge", [(0.01, False), (0.20, True)])
def test_depth_step(height, edge):
    """EDGE exactly for the corners whose window straddles a 20 % step; a 1 % step passes everywhere"""
    c, straddle = dc.step_case(height)
    z, status, rel = dc.restate(c)
    assert straddle.sum() == 6
    want = np.where(straddle & edge, dr.EDGE, dr.OK)
    assert np.array_equal(status, want), (status, want)
    # the relative range is measured against the centre: height on the near side, height / (1 + height) on the far side
    assert np.allclose(rel[straddle], np.where(c["xyl"][straddle, 0] < dc.STEP_COLUMN, height, height / (1 + height)), rtol=1e-6)
    assert np.all(rel[~straddle] == 0.0)


def test_defaults_and_zero_fields():
    assert dr.rule() == dr.DEFAULTS and dr.rule(min_valid=0, edge_ratio=0.0) == dr.DEFAULTS
    assert dr.rule(min_valid=5)["min_valid"] == 5 and dr.rule(max_depth=3.0)["max_depth"] == 3.0


def test_u16_scale():
    """a 16-bit image is its samples times the scale: zero is a hole, the depth is one multiplication"""
    d = np.full((48, 64), 7500, np.uint16)
    d[10, 10] = 0
    z, status, _ = dr.depth_seed(d, [(10, 10, 0), (20, 20, 1)], ol.TUM_CAM, scale=1.0 / 5000)
    assert list(status) == [dr.HOLE, dr.OK] and z[1] == 7500 * (1.0 / 5000)


def test_lens_centre_is_the_raw_pixel_of_the_ray(orc):
    """through the lens of config_tum_f2.cfg on `shelf`: for every OK corner the sampled depth is the analytic depth of the corner's
    undistorted ray against the surface it hits, within the largest difference between the sampled pixel and its four neighbours (the
    centre is the ray's raw pixel rounded: at most half a pixel off in each direction)"""
    c, scene = dc.lens_case(orc)
    z, status, _ = dc.restate(c)
    ok = np.flatnonzero(status == dr.OK)
    assert len(ok) >= 150, np.bincount(status, minlength=5)
    fu, fv = dr.centre_pixels(c["xyl"], c["cam"], c["dist"])
    plain_u, plain_v = dr.centre_pixels(c["xyl"], c["cam"], None)
    assert np.abs(fu - plain_u).max() > 3.0, "the lens moves corners by pixels: a centre without it would be another sample"
    fx, fy, u0, v0 = c["cam"]
    depth = c["depth"].astype(np.float64)
    h, w = depth.shape
    worst = 0.0
    for i in ok:
        x, y, l = [int(v) for v in c["xyl"][i]]
        want = dc.nearest_hit_depth(scene, ((x << l) - u0) / fx, ((y << l) - v0) / fy)
        cx, cy = int(fu[i]), int(fv[i])
        nb = [depth[cy, min(cx + 1, w - 1)], depth[cy, max(cx - 1, 0)], depth[min(cy + 1, h - 1), cx], depth[max(cy - 1, 0), cx]]
        tol = max(abs(v - depth[cy, cx]) for v in nb) + 1e-6      # (+ float32 depth at <= 2 m)
        assert abs(z[i] - want) <= tol, (i, z[i], want, tol)
        worst = max(worst, abs(z[i] - want))
    print("lens: %d OK corners, worst |sampled - analytic| %.3g m" % (len(ok), worst))


@pytest.mark.parametrize("i,k", dc.SHELF_FRAMES)
def test_shelf_counts(orc, i, k):
    """`shelf` without a lens: FAST fires on occlusion edges, the edge test takes those corners out and leaves enough to initialise"""
    c = dc.shelf_case(orc, i, k)
    z, status, rel = dc.restate(c)
    counts = np.bincount(status, minlength=5)
    print("shelf tracker %d frame %d: %d corners, OK %d EDGE %d FEW %d HOLE %d OUTSIDE %d; largest passing range %.3g, smallest rejected %.3g"
          % (i, k, len(status), counts[dr.OK], counts[dr.EDGE], counts[dr.FEW], counts[dr.HOLE], counts[dr.OUTSIDE],
             np.nanmax(rel[status == dr.OK]), np.nanmin(rel[status == dr.EDGE])))
    assert 240 <= counts[dr.OK] <= 270, counts
    assert 5 <= counts[dr.EDGE] <= 20, counts
    assert counts[dr.OK] >= 50          # SDVL.min_init_corners
    # OK corners carry a true surface's depth: the nearest hit of their own ray, to float32
    scene = sc_scene(orc, i, k)
    fx, fy, u0, v0 = c["cam"]
    for j in np.flatnonzero(status == dr.OK)[::7]:
        x, y, l = [int(v) for v in c["xyl"][j]]
        assert abs(z[j] - dc.nearest_hit_depth(scene, ((x << l) - u0) / fx, ((y << l) - v0) / fy)) <= 1e-6


def sc_scene(orc, i, k):
    import scene_cases as sc
    return sc.scene_synth().scene(ol.trajectory_pose(orc, k, sc.tracker_twist(i)), preset="shelf")
