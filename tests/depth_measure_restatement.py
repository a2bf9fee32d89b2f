"""The mapper's depth filter with a MEASURED depth (sdvl_depth_filter_measured, include/sdvl_hip.h) restated one candidate at a time in
plain Python floats, in the device's operation order: the SPECIFICATION of depth_filter_measured_kernel (csrc/sdvl_depth_filter.hip).  The rule is
this project's own.  It is composed of the two restatements it stands on, which are imported and not edited: depth_restatement (the loop
body of Map::UpdateCandidates, Point::Update, HasConverged and the SE3 arithmetic) and depth_seed_restatement (the validity of a depth
sample, the status codes, the rule's defaults).

  a miss                          depth_restatement.restate: Unpromote
  a hit at px, found level l      the depth lookup at px: centre floor(px + 0.5), with a lens floor(. + 0.5) of the raw pixel px's ray lands
                                  on (the forward model of cv::undistort in depth_seed_restatement's operation order); nine samples at
                                  stride 1 << l; OUTSIDE, HOLE, FEW, EDGE in that order, else OK with z_c the centre sample
  status not OK, or no image      depth_restatement.restate on the same inputs: the triangulated update
  status OK                       v = unproject(px), P_c = v (z_c / v.z), P_r = (ref cur^-1) P_c, depth = P_r . bearing: the range along the
                                  candidate's ray.  depth <= 0, depth < min_depth or depth < depth_mean scale_min_dist: SKIPPED.  No
                                  triangulation is made and no parallax test.  Otherwise Point::Update and HasConverged as in
                                  depth_restatement, with x = 1 / depth and tau = noise_abs + noise_quad (z_c z_c) in ComputeTau's place

restate(...) returns depth_restatement.restate's dict and `status`: the lookup's code, 255 where none was made.  fault=<name> plants one
error (FAULTS); ulps as in depth_restatement (behind a measured update only exp is left: ulps[4]).

Test infrastructure only."""
import math

import numpy as np

import depth_restatement as dr
import depth_seed_restatement as dsr
from depth_restatement import CONVERGED, FIXED_STALE, SKIPPED, UPDATED

NO_LOOKUP = 255
NOISE_DEFAULTS = dict(noise_abs=0.001, noise_quad=0.0015)

FAULTS = {
    "z_as_range": "the sample z_c is used as the range along the candidate's ray",
    "pose_swapped": "P_c is carried by cur * ref^-1 in place of ref * cur^-1",
    "stride_level0": "the window's stride is 1 at every level",
    "centre_truncated": "the centre is the truncated pixel, not floor(px + 0.5)",
    "tau_no_quad": "tau = noise_abs, without noise_quad z_c^2",
    "tau_quad_of_range": "the quadratic term takes the range, not z_c",
    "parallax_kept": "the parallax test of the triangulated rule is applied to the measured point",
    "no_depth_mean_test": "depth < depth_mean * scale_min_dist is not tested",
    "negative_depth_updates": "a range that is not positive is not skipped",
    "lens_ignored": "the centre is looked up at px itself although there is a lens",
    "edge_falls_to_ok": "an EDGE status updates from the sample all the same",
    "x_is_inverse_z": "the measurement is 1 / z_c, not 1 / depth",
}


def noise(noise_abs=0.0, noise_quad=0.0):
    """a field given as 0 takes its default, as in sdvl_depth_measure_params"""
    return dict(noise_abs=noise_abs if noise_abs != 0 else NOISE_DEFAULTS["noise_abs"],
                noise_quad=noise_quad if noise_quad != 0 else NOISE_DEFAULTS["noise_quad"])


def centre(px, cam, dist=None, fault=None):
    """-> (fu, fv): the centre sample's column and row before the range test, as floats"""
    u, v = float(px[0]), float(px[1])
    if dist is not None and float(dist[0]) != 0.0 and fault != "lens_ignored":
        fx, fy, u0, v0 = float(cam["fx"]), float(cam["fy"]), float(cam["u0"]), float(cam["v0"])
        k1, k2, p1, p2, k3 = [float(d) for d in dist]
        x, y = (u - u0) / fx, (v - v0) / fy
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
        v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
    if fault == "centre_truncated":
        return (float(math.trunc(u)) if math.isfinite(u) else u, float(math.trunc(v)) if math.isfinite(v) else v)
    return (math.floor(u + 0.5) if math.isfinite(u) else math.nan, math.floor(v + 0.5) if math.isfinite(v) else math.nan)


def lookup(depth, px, level, cam, dist=None, scale=1.0, rule=None, fault=None):
    """depth: [h, w] float32 or uint16 -> (status, z_c: the centre sample in metres as a float, 0.0 unless OK)"""
    r = dsr.rule(**(rule or {}))
    Z = dsr.metres(depth, scale)
    h, w = Z.shape
    fu, fv = centre(px, cam, dist, fault)
    if not (fu >= 0 and fu < w and fv >= 0 and fv < h):
        return dsr.OUTSIDE, 0.0
    cx, cy = int(fu), int(fv)
    s = 1 if fault == "stride_level0" else 1 << int(level)
    zc = float(Z[cy, cx])
    if not dsr.valid(Z[cy, cx], r):
        return dsr.HOLE, 0.0
    win = [float(Z[cy + j * s, cx + k * s]) for j in (-1, 0, 1) for k in (-1, 0, 1)
           if 0 <= cx + k * s < w and 0 <= cy + j * s < h and dsr.valid(Z[cy + j * s, cx + k * s], r)]
    if len(win) < r["min_valid"]:
        return dsr.FEW, 0.0
    if max(win) - min(win) > r["edge_ratio"] * zc:
        return (dsr.OK, zc) if fault == "edge_falls_to_ok" else (dsr.EDGE, 0.0)
    return dsr.OK, zc


def restate(cur_pose, ref_pose, bearing, found, px, level, cam, state, params, depth=None, dist=None, scale=1.0, rule=None, noise_abs=0.0,
            noise_quad=0.0, fault=None, ulps=(0, 0, 0, 0, 0)):
    """one candidate.  The first arguments as depth_restatement.restate's; level: the level the search found the point on; depth: the depth
    image of the current frame (None: the request is in no job); dist: (k1, k2, p1, p2, k3) or None; rule: fields of the lookup's rule"""
    assert fault is None or fault in FAULTS, fault
    tri = dict(cur_pose=cur_pose, ref_pose=ref_pose, bearing=bearing, found=found, px=px, cam=cam, state=state, params=params, ulps=ulps)
    if not found or depth is None:
        return dict(dr.restate(**tri), status=NO_LOOKUP)
    status, zc = lookup(depth, px, level, cam, dist, scale, rule, fault)
    if status != dsr.OK:
        return dict(dr.restate(**tri), status=status)
    nz = noise(noise_abs, noise_quad)
    cur, ref, fv = tuple(float(c) for c in cur_pose), tuple(float(c) for c in ref_pose), tuple(float(c) for c in bearing)
    st = state
    pi = 3.14159265
    out = dict(outcome=SKIPPED, n_failed=st["n_failed"], rho=st["rho"], sigma2=st["sigma2"], a=st["a"], b=st["b"], cos_alpha=None,
               last_distance=None, position=None, row={}, trace={}, status=status)
    trace = out["trace"]
    v3d = dr.unproject(cam, px)
    ref_world, cur_world = dr.se3_inverse(ref), dr.se3_inverse(cur)
    pose2 = dr.se3_mul(ref, dr.se3_inverse(cur))
    k = dr._div(zc, v3d[2])
    p_c = (v3d[0] * k, v3d[1] * k, v3d[2] * k)
    p_r = dr.se3_apply(dr.se3_mul(cur, dr.se3_inverse(ref)) if fault == "pose_swapped" else pose2, p_c)
    depth_r = zc if fault == "z_as_range" else dr.dot3(p_r, fv)
    tau = nz["noise_abs"] + (0.0 if fault == "tau_no_quad" else nz["noise_quad"] * ((depth_r * depth_r) if fault == "tau_quad_of_range" else (zc * zc)))
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


def tolerance(n_ulp=dr.N_ULP, **kw):
    """-> (the unmoved result, per float output the bound on |device - restatement|), derived as depth_restatement.tolerance derives its
    own, with its N_ULP, MARGIN and FLOOR_ULP.  A request that falls back to the triangulated update has that update's bound.  Behind a
    measured update only exp is left of the five transcendental calls: the bound is MARGIN times the larger movement of the output when
    exp's result is moved by +-n_ulp, plus FLOOR_ULP ulp of the value; an output with no transcendental behind it (the position of a
    fixed point, a skipped request's state) keeps the floor alone."""
    base = restate(**kw)
    if base["status"] != dsr.OK:
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
    """the outcomes a measured update meets when exp's result is moved by +-n_ulp (a designed case decides the same way in all three)"""
    return {restate(**dict(kw, ulps=(0, 0, 0, 0, k)))["outcome"] for k in (-n_ulp, 0, n_ulp)}
