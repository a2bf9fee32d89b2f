"""The cases of tests/test_gpu_depth_filter.py, shared with tests/test_depth_restatement_cpu.py and
tests/test_oracle_depth_independent.py.  Every case names what it is there for, and check(case) asserts, without a GPU, that the
restatement (tests/depth_restatement.py) gets there: the branch, the side of the threshold, the regime of tau.

Geometry.  TUM camera (fx 517.3, fy 516.5, u0 318.6, v0 255.3), max_failed 15, min_depth = scale_min_dist = 0.25.  A found case is
built around one world point P: the reference camera (centre, rotation) sees it at a chosen pixel, which gives the bearing, at a chosen
depth; the current camera's centre is placed where P sees the two centres under a chosen parallax angle phi, at `ratio` times the
reference camera's distance, in the half-plane named by an azimuth; it looks at a point beside P, so the found pixel lies off the
centre.  The found pixel is P's projection into the current camera unless the case moves it.

Decisions.  A case that asserts a decision keeps the deciding quantity at least 10 times that quantity's own spread under +-N_ULP on
the transcendental results away from the threshold (check() asserts it).  det, the triangulated depth and the parallax cosine of the
triangulated point have no transcendental in front of them: their spread is zero and the restatement has them in the device's
operation order; the cases still keep them a relative 1e-3 or more away from their thresholds (1e-8 absolute for the cosine, whose
rounding error is one or two units of 1e-16), except the early return, which lives in the last bit by its nature (see
_early_return_cases), and the two cases that put the depth ON a threshold (see _too_close_cases)."""
import math

import depth_restatement as dr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED

CAM = dict(width=640.0, height=480.0, fx=517.3, fy=516.5, u0=318.6, v0=255.3)
PARAMS = dict(px_error_angle=dr.pixel_error_angle(CAM["fx"]), min_depth=0.25, scale_min_dist=0.25, max_failed=15)
SEED = dict(sigma2=1.0, a=10.0, b=10.0, z_range=6.0)          # Point::InitCandidate (point.cc:50-60)


# ---------------------------------------------------------------------------------------------------- building blocks
def quat(axis, angle):
    n = math.sqrt(sum(c * c for c in axis))
    s = math.sin(0.5 * angle) / n
    return (math.cos(0.5 * angle), axis[0] * s, axis[1] * s, axis[2] * s)


def quat_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def pose_of(q, centre):
    """the world -> camera pose of a camera with rotation q (world -> camera) and the given centre: t = -R C"""
    rc = dr.mvec(dr.quat_to_rot(*q), centre)
    return tuple(q) + (-rc[0], -rc[1], -rc[2])


def look_at(centre, target, roll=0.0):
    """world -> camera rotation of a camera at `centre` whose optical axis passes through `target`, rolled about it"""
    z = _unit(_sub(target, centre))
    up = (0.0, 1.0, 0.0) if abs(z[1]) < 0.9 else (1.0, 0.0, 0.0)
    x = _unit(_cross(up, z))
    y = _cross(z, x)
    R = (x, y, z)                                              # rows: the camera's axes in world coordinates
    w = 0.5 * math.sqrt(max(0.0, 1.0 + R[0][0] + R[1][1] + R[2][2]))
    if w > 1e-3:
        q = (w, (R[2][1] - R[1][2]) / (4 * w), (R[0][2] - R[2][0]) / (4 * w), (R[1][0] - R[0][1]) / (4 * w))
    else:                                                      # a half turn: not used by any case
        raise ValueError("look_at: half turn")
    n = math.sqrt(sum(c * c for c in q))
    q = tuple(c / n for c in q)
    return quat_mul(quat((0.0, 0.0, 1.0), roll), q)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _unit(a):
    return _scale(a, 1.0 / dr.norm3(a))


def project(p):
    return (CAM["u0"] + CAM["fx"] * p[0] / p[2], CAM["v0"] + CAM["fy"] * p[1] / p[2])


def state(rho, sigma2=SEED["sigma2"], a=SEED["a"], b=SEED["b"], z_range=SEED["z_range"], cos_alpha=1.0, last_distance=None, depth_mean=0.5,
          position=(0.0, 0.0, 0.0), fixed=0, n_failed=0):
    return dict(rho=rho, sigma2=sigma2, a=a, b=b, z_range=z_range, cos_alpha=cos_alpha, last_distance=1.0 / rho if last_distance is None else last_distance,
                depth_mean=depth_mean, position=tuple(position), fixed=fixed, n_failed=n_failed)


def geometry(depth, phi, ratio=1.0, azimuth=0.3, ref_px=(250.0, 300.0), ref_centre=(0.4, -0.2, 0.1), ref_q=None, aim=(0.15, -0.1), roll=0.2):
    """-> dict(ref_pose, cur_pose, bearing, px, P): the point at `depth` along the bearing of ref_px, the current camera where P sees the two
    centres under the angle phi, at ratio * depth from P, looking at P + aim[0] e1 + aim[1] e2 (so that P lies off its axis)"""
    ref_q = quat((0.3, -0.5, 0.8), 0.4) if ref_q is None else ref_q
    ref_pose = pose_of(ref_q, ref_centre)
    bearing = dr.unproject(CAM, ref_px)
    P = dr.se3_apply(dr.se3_inverse(ref_pose), _scale(bearing, depth))
    u = _unit(_sub(ref_centre, P))
    e1 = _unit(_cross(u, (0.0, 0.0, 1.0) if abs(u[2]) < 0.9 else (1.0, 0.0, 0.0)))
    e2 = _cross(u, e1)
    w = _add(_scale(e1, math.cos(azimuth)), _scale(e2, math.sin(azimuth)))
    cur_centre = _add(P, _scale(_add(_scale(u, math.cos(phi)), _scale(w, math.sin(phi))), ratio * depth))
    target = _add(P, _add(_scale(e1, aim[0] * depth), _scale(e2, aim[1] * depth)))
    cur_pose = pose_of(look_at(cur_centre, target, roll), cur_centre)
    px = project(dr.se3_apply(cur_pose, P))
    return dict(ref_pose=ref_pose, cur_pose=cur_pose, bearing=bearing, px=px, P=P)


def case(name, purpose, geo, st, found=True, px=None, params=PARAMS, **want):
    """want: what check() asserts of the case: outcome=..., updated=True, position=..., regime=..., side=(quantity, '<' or '>=', threshold),
    exact=True (the quantity sits on the threshold)"""
    return dict(name=name, purpose=purpose, cur_pose=geo["cur_pose"], ref_pose=geo["ref_pose"], bearing=geo["bearing"], found=found,
                px=geo["px"] if px is None else px, state=st, params=params, want=want)


def inputs(c):
    return dict(cur_pose=c["cur_pose"], ref_pose=c["ref_pose"], bearing=c["bearing"], found=c["found"], px=c["px"], cam=CAM, state=c["state"],
                params=c["params"])


# ---------------------------------------------------------------------------------------------------- the cases
def _miss_cases():
    geo = geometry(2.0, 0.05)
    out = []
    for nf in (0, 14, 15, 16):
        gone = nf + 1 > 15
        out.append(case("miss-n_failed-%d" % nf, "Unpromote from n_failed = %d: b + 1, n_failed + 1, %s" % (nf, "deleted" if gone else "kept"), geo,
                        state(0.5, sigma2=0.04, a=12.5, b=7.25, cos_alpha=0.99, last_distance=2.1, n_failed=nf), found=False,
                        outcome=NOT_FOUND | (DELETED if gone else 0)))
    return out


def _no_triangulation_cases():
    """v_cur at the angle theta to R v_ref, turned out of the epipolar plane: det = sin^2 theta, and the least-squares depth is the
    foot of the current centre on the reference ray whatever theta is, so above the threshold the update runs on a sound triangle"""
    out = []
    for tag, theta in (("below", 1.0e-3 * 0.995), ("above", 1.0e-3 * 1.005)):
        geo = geometry(1.5, 0.4, ratio=0.8)
        pose = dr.se3_mul(geo["cur_pose"], dr.se3_inverse(geo["ref_pose"]))
        a0 = dr.mvec(dr.quat_to_rot(*pose[:4]), geo["bearing"])
        n = _unit(_cross(a0, pose[4:7]))
        a1 = _add(_scale(a0, math.cos(theta)), _scale(n, math.sin(theta)))
        want = dict(outcome=SKIPPED, side=("det", "<", 0.000001)) if tag == "below" else dict(updated=True, side=("det", ">=", 0.000001))
        out.append(case("no-triangulation-det-" + tag, "det = sin^2(%.4g) %s 1e-6" % (theta, tag), geo, state(1.0 / 1.3, sigma2=0.05), px=project(a1), **want))
    return out


def _no_parallax_cases():
    out = []
    limit = math.acos(0.999999)
    for tag, phi in (("skipped", limit * 0.99), ("passes", limit * 1.01)):
        want = dict(outcome=SKIPPED, side=("cos_alpha_tri", ">=", 0.999999)) if tag == "skipped" else dict(updated=True, side=("cos_alpha_tri", "<", 0.999999))
        out.append(case("no-parallax-" + tag, "parallax angle %.6g: cos_alpha on the %s side of 0.999999" % (phi, tag), geometry(2.0, phi),
                        state(1.0 / 2.1, sigma2=0.02), **want))
    return out


def _too_close_cases():
    out = []
    for tag, depth, mean, side in (("min_depth-below", 0.25 * 0.99, 0.5, ("depth", "<", 0.25)), ("min_depth-above", 0.25 * 1.01, 0.5, ("depth", ">=", 0.25)),
                                   ("depth_mean-below", 0.99, 4.0, ("depth", "<", 1.0)), ("depth_mean-above", 1.01, 4.0, ("depth", ">=", 1.0))):
        want = dict(outcome=SKIPPED) if tag.endswith("below") else dict(updated=True)
        out.append(case("too-close-" + tag, "depth %.4g against %s with depth_mean %.3g: that test alone decides" % (depth, side[2], mean),
                        geometry(depth, 0.05), state(1.0 / depth * 0.95, sigma2=0.05, depth_mean=mean), side=side, **want))
    # depth EQUAL to each threshold: both tests are `<`, so the update runs.  The triangulated depth has no transcendental in front of
    # it and the device computes it in the restatement's operation order, so min_depth (a parameter) and depth_mean (4 times it: the
    # product with 0.25 is exact) can be set to its very bits
    geo = geometry(0.7, 0.05, azimuth=2.2)
    d = dr.restate(cam=CAM, found=True, params=PARAMS, state=state(1.0), **{k: geo[k] for k in ("cur_pose", "ref_pose", "bearing", "px")})["trace"]["depth"]
    assert d / 0.25 * 0.25 == d and abs(d - 0.7) < 1e-12
    out.append(case("too-close-min_depth-equal", "depth == min_depth, bit for bit: not too close", geo, state(1.0 / 0.72, sigma2=0.05, depth_mean=0.5),
                    params=dict(PARAMS, min_depth=d), updated=True, side=("depth", ">=", d), exact=True))
    out.append(case("too-close-depth_mean-equal", "depth == depth_mean * scale_min_dist, bit for bit: not too close", geo,
                    state(1.0 / 0.72, sigma2=0.05, depth_mean=d / 0.25), updated=True, side=("depth", ">=", d), exact=True))
    return out


def _thin_parallax_cases():
    out = []
    for phi in (1.5e-3, 1.7e-3, 1.88e-3):
        out.append(case("negative-tau-%.2fmrad" % (phi * 1e3), "parallax %.3g rad under the pixel-error angle: gamma_plus < 0, tau < 0" % phi,
                        geometry(2.0, phi, azimuth=1.1), state(1.0 / 1.9, sigma2=0.03, a=11.0, b=12.0), updated=True, regime="negative-tau"))
    for phi in (1.97e-3, 2.4e-3, 2.95e-3):
        out.append(case("tau-clamp-%.2fmrad" % (phi * 1e3), "parallax %.3g rad just over the pixel-error angle: tau >= depth, the clamp acts" % phi,
                        geometry(3.0, phi, azimuth=-0.7), state(1.0 / 3.2, sigma2=0.03, a=14.0, b=10.5), updated=True, regime="clamp"))
    return out


def _regular_cases():
    """parallax x depth x sigma2 x (a, b) x distance of the measurement x z_range, as a covering set and not a product"""
    out = []
    grid = [  # phi, depth, sigma2, a, b, k (measurement k sqrt(sigma2) from rho), z_range, ref_px, azimuth
        (1e-2, 0.8, 1.0, 10.0, 10.0, 0.3, 6.0, (250.0, 300.0), 0.3),
        (1e-2, 6.0, 1e-3, 1.0, 1.0, 1.0, 6.0, (40.0, 60.0), 2.0),
        (3e-2, 2.0, 1.0, 10.0, 10.0, 10.0, 6.0, (600.0, 440.0), -1.0),
        (3e-2, 3.5, 1e-6, 300.0, 1.0, 3.0, 2.5, (320.0, 20.0), 0.9),
        (0.1, 1.2, 1e-9, 150.0, 150.0, 0.3, 6.0, (12.0, 470.0), 4.0),
        (0.1, 4.0, 1e-9, 300.0, 300.0, 1.0, 2.5, (500.0, 100.0), 5.5),
        (0.1, 2.5, 1e-9, 40.0, 3.0, 3.0, 6.0, (100.0, 250.0), 1.7),
        (0.1, 2.5, 1e-9, 40.0, 3.0, 10.0, 6.0, (100.0, 250.0), 1.7),
        (0.3, 0.8, 1e-3, 1.0, 300.0, 3.0, 6.0, (630.0, 240.0), 3.0),
        (0.3, 6.0, 1e-6, 300.0, 1.0, 10.0, 2.5, (330.0, 260.0), 0.1),
        (0.3, 1.7, 1.0, 1.0, 1.0, 10.0, 2.5, (200.0, 400.0), -2.2),
        (0.2, 5.0, 1e-6, 25.0, 270.0, 0.3, 6.0, (450.0, 50.0), 2.6),
        (5e-2, 1.0, 1e-3, 299.0, 1.0, 1.0, 2.5, (60.0, 200.0), -0.4),
        (2e-2, 3.0, 1e-9, 12.0, 288.0, 10.0, 6.0, (400.0, 300.0), 1.3),
    ]
    for i, (phi, depth, sigma2, a, b, k, z_range, ref_px, az) in enumerate(grid):
        geo = geometry(depth, phi, ratio=0.7 + 0.1 * (i % 5), azimuth=az, ref_px=ref_px, ref_q=quat((0.2 + 0.1 * i, -0.6, 0.4), 0.3 + 0.05 * i), roll=0.1 * i)
        rho = 1.0 / depth + k * math.sqrt(sigma2)
        out.append(case("regular-%02d" % i, "parallax %.3g, depth %.3g, sigma2 %.1g, a %.4g, b %.4g, measurement %.3g sigma from rho, z_range %.2g"
                        % (phi, depth, sigma2, a, b, k, z_range), geo, state(rho, sigma2=sigma2, a=a, b=b, z_range=z_range, depth_mean=depth, n_failed=i % 7),
                        updated=True, regime="regular"))
    return out


def _l_after(sigma2, geo, rho, **kw):
    return dr.restate(cam=CAM, found=True, params=PARAMS, state=state(rho, sigma2=sigma2, **kw), **{k: geo[k] for k in ("cur_pose", "ref_pose", "bearing", "px")})["trace"]["l"]


def _convergence_cases():
    out = []
    geo = geometry(2.0, 0.15, azimuth=0.8)
    rho, kw = 1.0 / 2.02, dict(a=30.0, b=8.0, cos_alpha=0.5, last_distance=2.2, n_failed=2)   # a previous cos_alpha that would decide otherwise
    lo, hi = 1e-8, 1.0                                          # the prior sigma2 whose posterior gives l = 0.1, by bisection (l grows with it)
    assert _l_after(lo, geo, rho, **kw) < 0.1 < _l_after(hi, geo, rho, **kw)
    for _ in range(100):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if _l_after(mid, geo, rho, **kw) < 0.1 else (lo, mid)
    for tag, s in (("below", lo * 0.9), ("above", lo * 1.1)):
        want = dict(outcome=CONVERGED, side=("l", "<", 0.1)) if tag == "below" else dict(outcome=UPDATED, side=("l", ">=", 0.1))
        out.append(case("convergence-l-" + tag, "l %s 0.1" % tag, geo, state(rho, sigma2=s, **kw), **want))
    fixed_at = (0.123, -4.5, 7.25)
    for tag, s in (("wide", 0.5), ("narrow", lo * 0.5)):
        out.append(case("convergence-fixed-" + tag, "fixed = 1 with a %s posterior: CONVERGED whatever l is, the position is state.position" % tag, geo,
                        state(rho, sigma2=s, position=fixed_at, fixed=1, **kw), outcome=CONVERGED, position=fixed_at,
                        side=("l", ">=" if tag == "wide" else "<", 0.1)))
    return out


_EARLY = {}


def _early_return_cases():
    """Update returns early when norm_scale is NaN (point.cc:74), and nothing but a NaN tau makes it so: acos of an argument outside
    [-1, 1].  The route: the current camera's centre ON the reference ray, so that the translation t of ref * cur^-1 is parallel to the
    bearing v and v.t / |t| is 1 up to rounding; both rays then meet in the current centre, the triangulated point is that centre up to
    rounding, and the parallax cosine seen from there is whatever the rounding of a vector of length ~1e-16 makes it (or NaN when it is
    exactly zero; NaN >= 0.999999 is false, so that passes).  The search: reference pixels on a grid, the current centre at distances
    0.5 .. 3.4 along the ray, until v.t / |t| comes out above 1 and every guard in front of Update passes.  Everything that decides is in
    front of the first transcendental call, so the device has the same bits."""
    if "cases" in _EARLY:
        return _EARLY["cases"]
    hits = []
    tried = 0
    ref_q, ref_centre = quat((0.3, -0.5, 0.8), 0.4), (0.4, -0.2, 0.1)
    ref_pose = pose_of(ref_q, ref_centre)
    for iu, iv, kd in ((iu, iv, kd) for iu in range(40) for iv in range(30) for kd in range(30)):
        if len(hits) == 2:
            break
        tried += 1
        ref_px, dist = (20.0 + 15.0 * iu, 15.0 + 15.0 * iv), 0.5 + 0.1 * kd
        bearing = dr.unproject(CAM, ref_px)
        cur_centre = dr.se3_apply(dr.se3_inverse(ref_pose), _scale(bearing, dist))
        cur_pose = pose_of(quat_mul(quat((0.1, 0.9, -0.2), 0.25), ref_q), cur_centre)
        geo = dict(ref_pose=ref_pose, cur_pose=cur_pose, bearing=bearing, px=(300.0 + iu, 200.0 + iv))
        t = dr.restate(cam=CAM, found=True, params=PARAMS, state=state(1.0 / dist, sigma2=0.04), **geo)["trace"]
        if t.get("arg_alpha", 0.0) > 1.0 and t["norm_scale"] != t["norm_scale"] and t["det"] > 1e-3:
            hits.append(geo)
    _EARLY["searched"] = tried
    out = []
    if len(hits) == 2:
        # the old state's l = 4 sqrt(sigma2) / rho^2 * cos_alpha / last_distance: 0.98 with sigma2 = 0.04, 0.0049 with sigma2 = 1e-6
        out.append(case("early-return-skipped", "norm_scale is NaN, the old state has l >= 0.1: SKIPPED, nothing changes", hits[0],
                        state(0.7, sigma2=0.04, a=17.0, b=4.0, cos_alpha=0.9, last_distance=1.5, n_failed=3), outcome=SKIPPED, regime="early-return",
                        side=("l", ">=", 0.1)))
        out.append(case("early-return-fixed-stale", "norm_scale is NaN, the old state has l < 0.1: fixed at the old estimate's position", hits[1],
                        state(0.7, sigma2=1e-6, a=17.0, b=4.0, cos_alpha=0.9, last_distance=1.5, n_failed=3), outcome=FIXED_STALE, regime="early-return",
                        side=("l", "<", 0.1)))
        out.append(case("early-return-already-fixed", "norm_scale is NaN and the point is fixed already: FIXED_STALE at state.position", hits[0],
                        state(0.7, sigma2=0.04, a=17.0, b=4.0, cos_alpha=0.9, last_distance=1.5, n_failed=3, position=(1.5, 2.5, -3.5), fixed=1),
                        outcome=FIXED_STALE, regime="early-return", position=(1.5, 2.5, -3.5)))
    _EARLY["cases"] = out
    return out


SEQUENCE_STEPS = 12


def sequence():
    """one candidate through SEQUENCE_STEPS updates of a widening baseline: -> the cases, each one's state the restatement's output of the one
    before.  The point lies at depth 2.5 and is seeded at 2.9; the parallax grows by 3.7 mrad a step, which leaves l at 0.105 after the
    eleventh update and takes it to 0.092 with the twelfth: only the last one converges"""
    out = []
    st = state(1.0 / 2.9, depth_mean=2.5)
    for k in range(SEQUENCE_STEPS):
        geo = geometry(2.5, 0.0037 * (k + 1), ratio=1.0 - 0.01 * k, azimuth=0.5 + 0.05 * k, ref_px=(410.0, 130.0))
        last = k == SEQUENCE_STEPS - 1
        c = case("sequence-%02d" % k, "update %d of %d of one candidate%s" % (k + 1, SEQUENCE_STEPS, ": converges" if last else ""), geo, st,
                 outcome=CONVERGED if last else UPDATED)
        out.append(c)
        o = dr.restate(**inputs(c))
        if o["position"] is None:
            break
        st = dict(st, rho=o["rho"], sigma2=o["sigma2"], a=o["a"], b=o["b"], cos_alpha=o["cos_alpha"], last_distance=o["last_distance"],
                  n_failed=o["n_failed"], fixed=1 if o["outcome"] == CONVERGED else st["fixed"],
                  position=o["position"] if o["outcome"] == CONVERGED else st["position"])
    return out


_ALL = {}


def all_cases():
    if "cases" not in _ALL:
        _ALL["cases"] = (_miss_cases() + _no_triangulation_cases() + _no_parallax_cases() + _too_close_cases() + _thin_parallax_cases() +
                         _regular_cases() + _convergence_cases() + _early_return_cases() + sequence())
        names = [c["name"] for c in _ALL["cases"]]
        assert len(set(names)) == len(names)
    return _ALL["cases"]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


_TOL = {}


def expected(c):
    """-> (the restatement's result, the bound per float output), computed once per case"""
    if c["name"] not in _TOL:
        _TOL[c["name"]] = dr.tolerance(**inputs(c))
    return _TOL[c["name"]]


def differences(c, got, with_row=True, skip=()):
    """what of a result `got` (a dict as restate returns it: the device's, the oracle's or a planted fault's) lies outside the case's
    expectation: the names of the integers, absent values and row fields that differ and of the floats beyond their bound, with
    (got, want, bound) each; and per float the ratio |got - want| / bound.  with_row = False: got has no row to look at; skip: names of
    floats that got does not have"""
    want, bound = expected(c)
    bad, ratio = {}, {}
    for k in ("outcome", "n_failed"):
        if got[k] != want[k]:
            bad[k] = (got[k], want[k], 0)
    gn, wn = dr._numbers(got), dr._numbers(want)
    if not with_row:
        gn, wn = ({k: v for k, v in d.items() if not k.startswith("row.")} for d in (gn, wn))
    for k in sorted((set(gn) | set(wn)) - set(skip)):
        if k not in gn or k not in wn:
            bad[k] = (gn.get(k), wn.get(k), None)
        elif wn[k] != wn[k] or gn[k] != gn[k]:
            if not (wn[k] != wn[k] and gn[k] != gn[k]):
                bad[k] = (gn[k], wn[k], None)
        else:
            d = abs(gn[k] - wn[k])
            ratio[k] = d / bound[k] if bound[k] > 0 else (0.0 if d == 0 else math.inf)
            if d > bound[k]:
                bad[k] = (gn[k], wn[k], bound[k])
    for k in ("n_failed", "fixed", "trash") if with_row else ():
        if got["row"].get(k) != want["row"].get(k):
            bad["row." + k] = (got["row"].get(k), want["row"].get(k), 0)
    return bad, ratio


# ---------------------------------------------------------------------------------------------------- a case is what it says
def check(c):
    """asserts, on the CPU, that the restatement takes the case where its name says, with the margins the module text states"""
    base, dev, tdev, outcomes = dr.spread(**inputs(c))
    want, t = c["want"], base["trace"]
    assert len(outcomes) == 1, (c["name"], "the outcome depends on the last bits of a transcendental", outcomes)
    if "outcome" in want:
        assert base["outcome"] == want["outcome"], (c["name"], base["outcome"], want["outcome"])
    if want.get("updated"):
        assert base["outcome"] in (UPDATED, CONVERGED), (c["name"], base["outcome"])
    if "position" in want:
        assert base["position"] == tuple(want["position"]), (c["name"], base["position"])
    if "side" in want:
        q, rel, thr = want["side"]
        v = t[q]
        assert (v < thr) if rel == "<" else (v >= thr), (c["name"], q, v, rel, thr)
        floor = 1e-8 if q == "cos_alpha_tri" else 1e-3 * thr
        if want.get("regime") == "early-return" or c["state"]["fixed"] or want.get("exact"):
            floor = 0.0                                           # l of an untouched or fixed point decides on a distance stated per case
        assert abs(v - thr) >= max(10.0 * tdev.get(q, 0.0), floor), (c["name"], q, v, thr, tdev.get(q))
    if base["outcome"] in (UPDATED, CONVERGED) and not c["state"]["fixed"]:
        # whatever the case is about, the convergence test behind its update is a decision too
        assert abs(t["l"] - 0.1) >= 10.0 * tdev["l"], (c["name"], "l", t["l"], tdev["l"])
    regime = want.get("regime")
    if regime in ("negative-tau", "clamp", "regular"):
        phi = math.acos(t["cos_alpha_tri"])
        assert 10.0 * tdev["tau"] < abs(t["tau"]), (c["name"], t["tau"], tdev["tau"])
    if regime == "negative-tau":
        assert 1.45e-3 < phi < 1.9e-3 and t["gamma_plus"] < 0.0 and t["tau"] < 0.0 and not t["clamped"], (c["name"], phi, t)
    if regime == "clamp":
        assert 1.95e-3 < phi < 3e-3 and t["tau"] >= t["depth"] and t["clamped"], (c["name"], phi, t)
        assert t["tau"] - t["depth"] > 10.0 * tdev["tau"], (c["name"], t["tau"], t["depth"], tdev["tau"])
    if regime == "regular":
        assert 0.9e-2 <= phi <= 0.31 and 0.79 <= t["depth"] <= 6.01 and t["tau"] > 0.0 and not t["clamped"], (c["name"], phi, t)
    if regime == "early-return":
        assert t["arg_alpha"] > 1.0 and t["norm_scale"] != t["norm_scale"], (c["name"], t)
        assert (base["rho"], base["sigma2"], base["a"], base["b"], base["n_failed"]) == tuple(c["state"][k] for k in ("rho", "sigma2", "a", "b", "n_failed"))
    return base
