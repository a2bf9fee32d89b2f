"""sdvl_stereo_lookup and the mapper's depth filter fed by it (sdvl_depth_filter_stereo, include/sdvl_hip.h) restated: the SPECIFICATION
of the kernels stereo_lookup (csrc/sdvl_stereo.hip) and of the filter's third form (csrc/sdvl_depth_filter.hip).  The rule is this
project's own.  It is composed of what is already stated, imported and not edited: stereo_restatement (`rule`, `call_range`, `costs`,
`parabola`: the matcher), depth_restatement (the triangulated update, Point::Update's arithmetic, the SE3 helpers).

The lookup.  A position px of the left image's level 0 (sub-pixel) found on level l:
  centre   (X, Y) = (floor(px + 0.5), floor(py + 0.5)); s = 1 << l; X need not be a multiple of s.  A position that is not finite: OUTSIDE
  then     stereo_restatement's rule at (X, Y, s), word for word: window, range (d_hi = min(d_cap, X - 4 s)), cost, ties, status order,
           parabola, z = fx b / disparity
  jobs     (left, right, begin, end): the positions begin .. end belong to that pair; a position in no job is NOMATCH

The filter.  One candidate:
  a miss, a hit in no job       depth_restatement.restate; status 255
  a hit at px on level l        the lookup at (px, l clamped to 0 .. 7)
  status not OK                 depth_restatement.restate on the same inputs: the same bits
  status OK with z_c            the measured update of depth_measure_restatement with noise_abs = 0 and noise_quad = disparity_sigma / (fx b):
                                from z = fx b / d, dz = z^2 / (fx b) dd, so tau = disparity_sigma z_c^2 / (fx b)
depth_measure_restatement.restate puts its default in for a noise field of 0, so the measured update is restated here for a general
(noise_abs, noise_quad); tests/test_stereo_lookup_restatement_cpu.py holds the copy bit-equal to the original where both can be called.
disparity_sigma 0 takes 0.25 px: an order of magnitude that nobody has measured against a real pair (on `shelf` the matcher's median
error is 0.04 - 0.07 px).

fault=<name> plants one error (FAULTS); ulps as in depth_restatement.

Test infrastructure only."""
import math

import numpy as np

import depth_restatement as dr
import stereo_restatement as sr
from depth_restatement import CONVERGED, FIXED_STALE, SKIPPED, UPDATED
from stereo_restatement import AMBIGUOUS, EDGE, HALF, MAX_LEVELS, NOMATCH, OK, OUTSIDE, Refused  # noqa: F401

NO_LOOKUP = 255
DISPARITY_SIGMA = 0.25      # what disparity_sigma 0 stands for; not measured against a real pair

FAULTS = {
    "centre_truncated": "the centre is the truncated pixel, not floor(px + 0.5)",
    "centre_on_grid": "the centre is pulled onto the level's grid: (X // s) s",
    "stride_level0": "the window's stride is 1 at every level",
    "range_of_grid": "d_hi takes X // s * s - 4 s, not X - 4 s",
    "edge_falls_to_ok": "an EDGE status updates from the match all the same",
    "tau_linear": "tau = disparity_sigma z_c / (fx b): z_c not squared",
    "tau_no_baseline": "tau = disparity_sigma z_c^2 / fx: the baseline left out",
    "tau_depth_default": "noise_abs 0 takes the depth camera's default 0.001 m",
    "sigma_default_ignored": "disparity_sigma 0 is taken as 0, not as 0.25 px",
    "z_as_range": "the depth z_c is used as the range along the candidate's ray",
    "pose_swapped": "P_c is carried by cur * ref^-1 in place of ref * cur^-1",
    "parallax_kept": "the parallax test of the triangulated rule is applied to the measured point",
    "no_depth_mean_test": "depth < depth_mean * scale_min_dist is not tested",
    "negative_depth_updates": "a range that is not positive is not skipped",
    "x_is_inverse_z": "the measurement is 1 / z_c, not 1 / depth",
}


def centre(px, fault=None):
    """-> (X, Y) as floats, NaN for a coordinate that is not finite"""
    out = []
    for c in (float(px[0]), float(px[1])):
        if not math.isfinite(c):
            out.append(math.nan)
        else:
            out.append(float(math.trunc(c)) if fault == "centre_truncated" else float(math.floor(c + 0.5)))
    return tuple(out)


def match_at(left, right, X, Y, s, fb, d_lo, d_cap, r, fault=None):
    """stereo_restatement's rule at the level-0 centre (X, Y) with the stride s -> (status, disparity, z)"""
    h, w = left.shape
    if X - HALF * s < 0 or X + HALF * s >= w or Y - HALF * s < 0 or Y + HALF * s >= h:
        return OUTSIDE, 0.0, 0.0
    d_hi = min(d_cap, (X // s * s if fault == "range_of_grid" else X) - HALF * s)
    if d_hi - d_lo + 1 < 3:
        return OUTSIDE, 0.0, 0.0
    c = sr.costs(left, right, X, Y, s, d_lo, d_hi)
    best = [int(np.argmin(c[k])) for k in range(5)]
    i0 = best[0]
    S0 = int(c[0, i0])
    if S0 > 81 * r["max_sad"] or i0 == 0 or i0 == d_hi - d_lo:
        return NOMATCH, 0.0, 0.0
    far = np.abs(np.arange(d_hi - d_lo + 1) - i0) > 1
    if far.any() and 100 * S0 > r["uniqueness"] * int(c[0, far].min()):
        return AMBIGUOUS, 0.0, 0.0
    if any(abs(b - i0) > 1 for b in best[1:]) and fault != "edge_falls_to_ok":
        return EDGE, 0.0, 0.0
    disp = np.float64(d_lo + i0) + sr.parabola(c[0, i0 - 1], S0, c[0, i0 + 1])
    return OK, float(disp), float(fb / disp)


def lookup(left, right, px, level, cam, baseline, fault=None, **kw):
    """one position of one pair -> (status, disparity, z); cam = (fx, fy, u0, v0)"""
    r = sr.rule(baseline, **kw)
    fb, d_lo, d_cap = sr.call_range(cam[0], r)
    h, w = left.shape
    fu, fv = centre(px, fault)
    if not (fu >= 0 and fu < w and fv >= 0 and fv < h):
        return OUTSIDE, 0.0, 0.0
    s = 1 if fault == "stride_level0" else 1 << int(level)
    X, Y = int(fu), int(fv)
    if fault == "centre_on_grid":
        X, Y = X // s * s, Y // s * s
    return match_at(left, right, X, Y, s, fb, d_lo, d_cap, r, fault)


def stereo_lookup(jobs, px, levels, cam, baseline, dist=None, pyramid_levels=5, **kw):
    """the entry's call: jobs = [(left, right, begin, end), ...] over one position list -> (z, disparity, status, ok per job)"""
    if dist is not None and float(dist[0]) != 0.0:
        raise Refused("a lens: rectified pairs only")
    sr.rule(baseline, **kw)
    px = np.asarray(px, np.float64).reshape(-1, 2)
    levels = np.asarray(levels, np.int64).reshape(-1)
    n = len(px)
    if len(levels) != n:
        raise Refused("one level per position")
    named = np.zeros(n, bool)
    for left, right, b, e in jobs:
        sr.check_inputs(left, right, np.zeros((0, 3)), pyramid_levels)
        if not 0 <= b <= e <= n:
            raise Refused("position range outside the position list")
        if named[b:e].any():
            raise Refused("position ranges overlap")
        named[b:e] = True
        if e > b and not ((levels[b:e] >= 0).all() and (levels[b:e] < pyramid_levels).all()):
            raise Refused("a position's level lies outside the left frame's pyramid")
    z, disp, status, ok = np.zeros(n), np.zeros(n), np.full(n, NOMATCH, np.uint8), []
    for left, right, b, e in jobs:
        for i in range(b, e):
            status[i], disp[i], z[i] = lookup(np.asarray(left), np.asarray(right), px[i], levels[i], cam, baseline, **kw)
        ok.append(int((status[b:e] == OK).sum()))
    return z, disp, status, np.array(ok, np.int32)


def sigma_of(disparity_sigma=0.0, fault=None):
    """0 takes the default; negative or not finite is refused"""
    s = float(disparity_sigma)
    if not (math.isfinite(s) and s >= 0.0):
        raise Refused("disparity_sigma negative or not finite")
    return s if s != 0.0 or fault == "sigma_default_ignored" else DISPARITY_SIGMA


def stereo_noise(cam, baseline, disparity_sigma=0.0, fault=None):
    """-> (noise_abs, noise_quad) of the measured update: exactly 0 and disparity_sigma / (fx b)"""
    fb = float(np.float64(cam["fx"]) * np.float64(baseline))
    quad = dr._div(sigma_of(disparity_sigma, fault), float(cam["fx"]) if fault == "tau_no_baseline" else fb)
    return (0.001 if fault == "tau_depth_default" else 0.0), quad


def measured_update(cur_pose, ref_pose, bearing, px, cam, state, params, zc, noise_abs, noise_quad, fault=None, ulps=(0, 0, 0, 0, 0)):
    """depth_measure_restatement's measured update for a depth z_c at px and a general (noise_abs, noise_quad), neither replaced by a
    default: tau = noise_abs + noise_quad (z_c z_c).  -> depth_restatement.restate's dict, without `status`"""
    cur, ref, fv = tuple(float(c) for c in cur_pose), tuple(float(c) for c in ref_pose), tuple(float(c) for c in bearing)
    st = state
    pi = 3.14159265
    out = dict(outcome=SKIPPED, n_failed=st["n_failed"], rho=st["rho"], sigma2=st["sigma2"], a=st["a"], b=st["b"], cos_alpha=None,
               last_distance=None, position=None, row={}, trace={})
    trace = out["trace"]
    v3d = dr.unproject(cam, px)
    ref_world, cur_world = dr.se3_inverse(ref), dr.se3_inverse(cur)
    pose2 = dr.se3_mul(ref, dr.se3_inverse(cur))
    k = dr._div(zc, v3d[2])
    p_c = (v3d[0] * k, v3d[1] * k, v3d[2] * k)
    p_r = dr.se3_apply(dr.se3_mul(cur, dr.se3_inverse(ref)) if fault == "pose_swapped" else pose2, p_c)
    depth_r = zc if fault == "z_as_range" else dr.dot3(p_r, fv)
    tau = noise_abs + noise_quad * (zc if fault == "tau_linear" else (zc * zc))
    trace.update(z=zc, depth=depth_r, tau=tau, p_r=p_r)
    if not (depth_r > 0.0) and fault != "negative_depth_updates":
        return out
    if fault == "parallax_kept":
        p3d = dr.se3_apply(ref_world, (depth_r * fv[0], depth_r * fv[1], depth_r * fv[2]))
        if dr.parallax(ref_world[4:7], cur_world[4:7], p3d) >= 0.999999:
            return out
    too_close = depth_r < params["min_depth"]
    if fault != "no_depth_mean_test":
        too_close = too_close or depth_r < st["depth_mean"] * params["scale_min_dist"]
    if too_close:
        return out

    def position(rho):                                                      # Point::GetPosition, point.cc:128-142
        if st["fixed"]:
            return tuple(st["position"])
        sc = 1.0 / rho
        return dr.se3_apply(ref_world, (sc * fv[0], sc * fv[1], sc * fv[2]))

    def has_converged(sigma2, rho, cos_alpha, last_distance):               # Point::HasConverged, point.cc:162-176
        std_d = dr._div(math.sqrt(sigma2), rho * rho)
        l = dr._div(4 * std_d * cos_alpha, last_distance)
        trace["l"] = l
        return bool(st["fixed"]) or l < 0.1

    # Point::Update, point.cc:63-100, tau given
    gap = depth_r - tau
    trace["clamped"] = not (gap > 0.0000001)
    gap = 0.0000001 if not (gap > 0.0000001) else gap
    tau_inverse = 0.5 * (dr._div(1.0, gap) - dr._div(1.0, depth_r + tau))
    tau2 = tau_inverse * tau_inverse
    x = dr._div(1., zc) if fault == "x_is_inverse_z" else dr._div(1., depth_r)
    norm_scale = math.sqrt(st["sigma2"] + tau2) if st["sigma2"] + tau2 >= 0 else math.nan
    trace.update(tau2=tau2, norm_scale=norm_scale, x=x)
    if norm_scale != norm_scale:
        if has_converged(st["sigma2"], st["rho"], st["cos_alpha"], st["last_distance"]):
            pos = position(st["rho"])
            out.update(outcome=FIXED_STALE, cos_alpha=st["cos_alpha"], last_distance=st["last_distance"], position=pos)
            out["row"] = dict(P=pos, fixed=1)
        return out
    sigma2, rho, a, b, z_range = st["sigma2"], st["rho"], st["a"], st["b"], st["z_range"]
    s2 = 1. / (1. / sigma2 + dr._div(1., tau2))
    m = s2 * (rho / sigma2 + dr._div(x, tau2))
    C1 = a / (a + b) * dr.pdf_normal(rho, norm_scale, x, pi, ulps[4])
    C2 = b / (a + b) * 1. / z_range
    normalization_constant = C1 + C2
    C1 /= normalization_constant
    C2 /= normalization_constant
    f = C1 * (a + 1.) / (a + b + 1.) + C2 * a / (a + b + 1.)
    e = C1 * (a + 1.) * (a + 2.) / ((a + b + 1.) * (a + b + 2.)) + C2 * a * (a + 1.0) / ((a + b + 1.0) * (a + b + 2.0))
    rho_new = C1 * m + C2 * rho
    sigma2_new = C1 * (s2 + m * m) + C2 * (sigma2 + rho * rho) - rho_new * rho_new
    a_new = (e - f) / (f - e / f)
    b_new = a_new * (1.0 - f) / f
    trace.update(C1=C1, C2=C2, s2=s2, m=m, f=f, e=e)
    pos = position(rho_new)
    cos_alpha = dr.parallax(ref_world[4:7], cur_world[4:7], pos)
    last_distance = dr.norm3((cur_world[4] - pos[0], cur_world[5] - pos[1], cur_world[6] - pos[2]))
    conv = has_converged(sigma2_new, rho_new, cos_alpha, last_distance)
    out.update(outcome=CONVERGED if conv else UPDATED, n_failed=0, rho=rho_new, sigma2=sigma2_new, a=a_new, b=b_new, cos_alpha=cos_alpha,
               last_distance=last_distance, position=pos)
    out["row"] = dict(P=pos, idepth=rho_new, idepth_std=math.sqrt(sigma2_new), n_failed=0)
    if conv:
        out["row"]["fixed"] = 1
    return out


def restate(cur_pose, ref_pose, bearing, found, px, level, cam, state, params, pair=None, baseline=None, disparity_sigma=0.0, rule=None,
            fault=None, ulps=(0, 0, 0, 0, 0)):
    """one candidate.  The first arguments as depth_restatement.restate's (cam a dict); level: the level the search found the point on;
    pair: (left, right) of the current frame (None: the request is in no job); rule: fields of the matcher's rule
    -> depth_restatement.restate's dict and `status` (the lookup's code, 255 where none was made), `disparity`"""
    assert fault is None or fault in FAULTS, fault
    tri = dict(cur_pose=cur_pose, ref_pose=ref_pose, bearing=bearing, found=found, px=px, cam=cam, state=state, params=params, ulps=ulps)
    if not found or pair is None:
        return dict(dr.restate(**tri), status=NO_LOOKUP, disparity=0.0)
    noise_abs, noise_quad = stereo_noise(cam, baseline, disparity_sigma, fault)
    l = min(max(int(level), 0), MAX_LEVELS - 1)
    cam4 = (cam["fx"], cam["fy"], cam["u0"], cam["v0"])
    status, disp, zc = lookup(np.asarray(pair[0]), np.asarray(pair[1]), px, l, cam4, baseline, fault, **(rule or {}))
    if status != OK:
        return dict(dr.restate(**tri), status=status, disparity=0.0)
    out = measured_update(cur_pose, ref_pose, bearing, px, cam, state, params, zc, noise_abs, noise_quad, fault, ulps)
    return dict(out, status=status, disparity=disp)


def tolerance(n_ulp=dr.N_ULP, **kw):
    """depth_measure_restatement.tolerance's scheme on this restatement -> (the unmoved result, per float output the bound on
    |device - restatement|): a request that falls back has the triangulated update's bound; behind a measured update only exp is left,
    moved by +-n_ulp, times MARGIN, plus FLOOR_ULP ulp of the value"""
    base = restate(**kw)
    if base["status"] != OK:
        tri = {k: kw[k] for k in ("cur_pose", "ref_pose", "bearing", "found", "px", "cam", "state", "params")}
        _, bound = dr.tolerance(n_ulp, **tri)
        return base, bound
    b_num = dr._numbers(base)
    dev = dict.fromkeys(b_num, 0.0)
    if base["outcome"] in (UPDATED, CONVERGED):
        for k_exp in (-n_ulp, n_ulp):
            o = restate(**dict(kw, ulps=(0, 0, 0, 0, k_exp)))
            assert o["outcome"] in (UPDATED, CONVERGED)
            for k, v in dr._numbers(o).items():
                dev[k] = max(dev[k], abs(v - b_num[k]))
    return base, {k: dr.MARGIN * dev[k] + dr.FLOOR_ULP * math.ulp(v) if v == v and not math.isinf(v) else 0.0 for k, v in b_num.items()}


def spread_outcomes(n_ulp=dr.N_ULP, **kw):
    """the outcomes a measured update meets when exp's result is moved by +-n_ulp"""
    return {restate(**dict(kw, ulps=(0, 0, 0, 0, k)))["outcome"] for k in (-n_ulp, 0, n_ulp)}
