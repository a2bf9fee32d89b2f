"""The body of Map::UpdateCandidates' loop behind SearchPoint (map.cc:454-497) with Point::Update, Unpromote, GetPosition, HasConverged,
ComputeTau and PDFNormal (point.cc:64-118, 128-142, 164-217) and GetDepthFromTriangulation / GetParallax (extra/utils.cc:193-213),
restated one candidate at a time in plain Python floats from the reference's text: what tests/test_gpu_depth_filter.py holds
depth_filter_kernel against, and tests/test_oracle_depth_independent.py the oracle's sdvl_ref_depth_filter.

Only `math` and floats.  Python evaluates a float expression in the order it is written, without fusing, so every quantity in front of
the first transcendental call (quaternion to rotation, the pose products, the triangulation, the parallax) is written here in the
operation order the device code is built with (csrc/sdvl_math.h) and can be expected to agree with it to the last bits; behind
acos / sin / exp the device library's last bits differ from libm's, and the tolerance of a comparison comes from tolerance() below.

restate(...) returns dict(outcome, n_failed, rho, sigma2, a, b, cos_alpha, last_distance, position, row, trace):
  outcome        as include/sdvl_hip.h numbers it: NOT_FOUND 0 (| DELETED 0x100), SKIPPED 1, UPDATED 2, CONVERGED 3, FIXED_STALE 4
  cos_alpha, last_distance, position
                 of the point after the call where the outcome is UPDATED / CONVERGED / FIXED_STALE, else None
  row            what the point's row in the tracking tables receives: a dict with some of P, idepth, idepth_std, n_failed, fixed
                 (values) and trash (True); a field that is absent stays as it was
  trace          the deciding quantities: det, cos_alpha_tri, depth, tau, clamped, norm_scale, C1, l, ...
fault=<name> plants exactly one error (FAULTS).  ulps=(k0..k4) moves the results of the five transcendental calls of an update, in
the order acos(alpha), acos(beta), sin(beta_plus), sin(gamma_plus), exp, by that many units in the last place each."""
import math

NOT_FOUND, SKIPPED, UPDATED, CONVERGED, FIXED_STALE, DELETED = 0, 1, 2, 3, 4, 0x100
TRANSCENDENTALS = ("acos_alpha", "acos_beta", "sin_beta_plus", "sin_gamma_plus", "exp")

FAULTS = {
    "miss_b_kept": "Unpromote leaves b as it was (point.cc:111)",
    "delete_ge": "n_failed >= max_failed deletes, in place of > (point.cc:112)",
    "tau_inverse_pose": "ComputeTau is given cur * ref^-1 in place of ref * cur^-1 (point.cc:67)",
    "no_clamp": "depth - tau goes into tau_inverse without max(0.0000001, .) (point.cc:69)",
    "no_depth_mean_test": "only depth < min_depth is tested, depth < depth_mean * scale_min_dist is not (map.cc:482)",
    "exact_pi": "math.pi in place of 3.14159265 (point.cc:187, :201)",
    "position_old_rho": "the position after an update is taken at the old inverse depth (point.cc:91, :96)",
    "fixed_recomputed": "the position of a fixed point is recomputed from its inverse depth (point.cc:135)",
    "n_failed_kept": "an update leaves n_failed as it was (point.cc:99)",
    "converge_prev_cos": "HasConverged reads the cos_alpha of the previous update (point.cc:97, :167)",
    "row_std_sigma2": "the row's idepth_std receives sigma2 in place of its root (Point::GetStd)",
    "row_fixed_on_updated": "the row's fixed is set by every update, converged or not",
    "row_trash_every_miss": "the row is marked trash by every miss, deleted or not",
}


# ------------------------------------------------------------------------------------------------ SE3 (extra/se3.h, se3.cc)
def quat_to_rot(w, x, y, z):
    """Eigen::Quaterniond::toRotationMatrix (se3.h:41), row-major 9-tuple"""
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return (1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy))


def mvec(R, v):
    return (R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2], R[6] * v[0] + R[7] * v[1] + R[8] * v[2])


def se3_inverse(T):
    """SE3::Inverse (se3.cc:59-70): the inverse quaternion, -R^-1 t"""
    q0, q1, q2, q3 = T[:4]
    n2 = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3
    r = (q0 / n2, -q1 / n2, -q2 / n2, -q3 / n2) if n2 > 0.0 else (0.0, 0.0, 0.0, 0.0)
    rt = mvec(quat_to_rot(*r), T[4:7])
    return r + (-rt[0], -rt[1], -rt[2])


def se3_mul(A, B):
    """SE3::operator* (se3.cc:166-177): the normalised quaternion product, A.t + R(A) B.t"""
    a0, a1, a2, a3 = A[:4]
    b0, b1, b2, b3 = B[:4]
    w = a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3
    x = a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2
    y = a0 * b2 + a2 * b0 + a3 * b1 - a1 * b3
    z = a0 * b3 + a3 * b0 + a1 * b2 - a2 * b1
    n = math.sqrt(w * w + x * x + y * y + z * z)
    m = mvec(quat_to_rot(a0, a1, a2, a3), B[4:7])
    return (w / n, x / n, y / n, z / n, A[4] + m[0], A[5] + m[1], A[6] + m[2])


def se3_apply(T, p):
    """SE3 * Vector3d (se3.h:68)"""
    m = mvec(quat_to_rot(*T[:4]), p)
    return (m[0] + T[4], m[1] + T[5], m[2] + T[6])


def norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def unproject(cam, px):
    """Camera::Unproject (camera.cc:75-79): the unit bearing of a pixel"""
    v = ((px[0] - cam["u0"]) / cam["fx"], (px[1] - cam["v0"]) / cam["fy"], 1.0)
    n = norm3(v)
    return (v[0] / n, v[1] / n, v[2] / n)


def pixel_error_angle(fx):
    """Camera::GetPixelErrorAngle (camera.h:104-107)"""
    return math.atan(1.0 / (2.0 * fx)) * 2.0


# ------------------------------------------------------------------------------------------------ extra/utils.cc:193-213
def depth_from_triangulation(pose, v_ref, v_cur):
    """-> (det, depth or None): A = [R v_ref | v_cur], depth2 = -(A^T A)^-1 A^T t, |depth2[0]|; None when det < 0.000001"""
    a0 = mvec(quat_to_rot(*pose[:4]), v_ref)
    a1 = v_cur
    m00, m01, m11 = dot3(a0, a0), dot3(a0, a1), dot3(a1, a1)
    det = m00 * m11 - m01 * m01
    if det < 0.000001:
        return det, None
    invdet = 1.0 / det
    i00, i01 = m11 * invdet, -m01 * invdet
    n00, n01 = -i00, -i01
    r0 = (n00 * a0[0] + n01 * a1[0], n00 * a0[1] + n01 * a1[1], n00 * a0[2] + n01 * a1[2])
    return det, abs(r0[0] * pose[4] + r0[1] * pose[5] + r0[2] * pose[6])


def parallax(src1, src2, p3d):
    """GetParallax: the cosine of the angle under which p3d sees the two positions"""
    v1 = (src1[0] - p3d[0], src1[1] - p3d[1], src1[2] - p3d[2])
    v2 = (src2[0] - p3d[0], src2[1] - p3d[1], src2[2] - p3d[2])
    n1, n2 = norm3(v1), norm3(v2)
    v1 = tuple(_div(c, n1) for c in v1)
    v2 = tuple(_div(c, n2) for c in v2)
    return dot3(v1, v2)


def _div(a, b):
    """IEEE division: x / 0 is an infinity or NaN, where Python raises"""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _moved(x, k):
    """x moved by k units in the last place (NaN and infinities stay)"""
    if x != x or math.isinf(x):
        return x
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def _acos(x):
    return math.acos(x) if -1.0 <= x <= 1.0 else math.nan      # libm's answer outside the domain, where Python raises


def _sin(x):
    return math.sin(x) if math.isfinite(x) else math.nan


def _exp(x):
    if x != x:
        return x
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


# ------------------------------------------------------------------------------------------------ point.cc
def compute_tau(pose, v, depth, px_error_angle, pi, ulps, trace):
    """Point::ComputeTau, point.cc:186-198"""
    t = pose[4:7]
    a = (v[0] * depth - t[0], v[1] * depth - t[1], v[2] * depth - t[2])
    t_norm, a_norm = norm3(t), norm3(a)
    arg_alpha = _div(v[0] * t[0] + v[1] * t[1] + v[2] * t[2], t_norm)
    arg_beta = _div(a[0] * -t[0] + a[1] * -t[1] + a[2] * -t[2], t_norm * a_norm)
    alpha = _moved(_acos(arg_alpha), ulps[0])
    beta = _moved(_acos(arg_beta), ulps[1])
    beta_plus = beta + px_error_angle
    gamma_plus = pi - alpha - beta_plus
    depth_plus = _div(t_norm * _moved(_sin(beta_plus), ulps[2]), _moved(_sin(gamma_plus), ulps[3]))
    trace.update(arg_alpha=arg_alpha, arg_beta=arg_beta, alpha=alpha, beta=beta, gamma_plus=gamma_plus)
    return depth_plus - depth


def pdf_normal(mean, sd, x, pi, ulp_exp):
    """Point::PDFNormal, point.cc:200-215"""
    result = 0.0
    if sd <= 0:
        return result
    exponent = x - mean
    exponent *= -exponent
    exponent /= 2 * sd * sd
    result = _moved(_exp(exponent), ulp_exp)
    result /= sd * math.sqrt(2.0 * pi)
    return result


def restate(cur_pose, ref_pose, bearing, found, px, cam, state, params, fault=None, ulps=(0, 0, 0, 0, 0)):
    """one candidate through the loop body.  cur_pose / ref_pose: world -> camera, (qw, qx, qy, qz, tx, ty, tz); bearing: of the
    candidate's first observation, in the reference frame; found / px: SearchPoint's answer; cam: dict(fx, fy, u0, v0); state:
    dict(rho, sigma2, a, b, z_range, cos_alpha, last_distance, depth_mean, position, fixed, n_failed); params: dict(px_error_angle,
    min_depth, scale_min_dist, max_failed)"""
    assert fault is None or fault in FAULTS, fault
    cur, ref, fv = tuple(float(c) for c in cur_pose), tuple(float(c) for c in ref_pose), tuple(float(c) for c in bearing)
    st = state
    pi = math.pi if fault == "exact_pi" else 3.14159265
    out = dict(outcome=SKIPPED, n_failed=st["n_failed"], rho=st["rho"], sigma2=st["sigma2"], a=st["a"], b=st["b"], cos_alpha=None,
               last_distance=None, position=None, row={}, trace={})
    trace = out["trace"]
    if not found:
        # Point::Unpromote, point.cc:109-116; Map::DeletePoint when it says so (map.cc:459-460)
        out["n_failed"] = st["n_failed"] + 1
        if fault != "miss_b_kept":
            out["b"] = st["b"] + 1.0
        gone = out["n_failed"] >= params["max_failed"] if fault == "delete_ge" else out["n_failed"] > params["max_failed"]
        out["outcome"] = NOT_FOUND | (DELETED if gone else 0)
        out["row"] = dict(n_failed=out["n_failed"])
        if gone or fault == "row_trash_every_miss":
            out["row"]["trash"] = True
        return out

    pose = se3_mul(cur, se3_inverse(ref))                                   # map.cc:466
    v3d = unproject(cam, px)
    det, depth = depth_from_triangulation(pose, fv, v3d)
    trace.update(det=det, depth=depth)
    if depth is None:
        return out
    ref_world, cur_world = se3_inverse(ref), se3_inverse(cur)               # Frame::GetWorldPose
    p3d = se3_apply(ref_world, (depth * fv[0], depth * fv[1], depth * fv[2]))
    cos_tri = parallax(ref_world[4:7], cur_world[4:7], p3d)
    trace["cos_alpha_tri"] = cos_tri
    if cos_tri >= 0.999999:                                                 # map.cc:476
        return out
    too_close = depth < params["min_depth"]
    if fault != "no_depth_mean_test":
        too_close = too_close or depth < st["depth_mean"] * params["scale_min_dist"]
    if too_close:                                                           # map.cc:482
        return out

    def position(rho):                                                      # Point::GetPosition, point.cc:128-142
        if st["fixed"] and fault != "fixed_recomputed":
            return tuple(st["position"])
        sc = 1.0 / rho
        return se3_apply(ref_world, (sc * fv[0], sc * fv[1], sc * fv[2]))

    def has_converged(sigma2, rho, cos_alpha, last_distance):               # Point::HasConverged, point.cc:162-176
        std_d = _div(math.sqrt(sigma2), rho * rho)
        l = _div(4 * std_d * cos_alpha, last_distance)
        trace["l"] = l
        return bool(st["fixed"]) or l < 0.1

    # Point::Update, point.cc:63-100
    pose2 = pose if fault == "tau_inverse_pose" else se3_mul(ref, se3_inverse(cur))
    tau = compute_tau(pose2, fv, depth, params["px_error_angle"], pi, ulps, trace)
    gap = depth - tau
    trace.update(tau=tau, clamped=not (gap > 0.0000001))
    if fault != "no_clamp":
        gap = 0.0000001 if not (gap > 0.0000001) else gap                   # std::max(0.0000001, x): a NaN x stays out
    tau_inverse = 0.5 * (_div(1.0, gap) - _div(1.0, depth + tau))
    tau2 = tau_inverse * tau_inverse
    x = 1. / depth
    norm_scale = math.sqrt(st["sigma2"] + tau2) if st["sigma2"] + tau2 >= 0 else math.nan
    trace.update(tau2=tau2, norm_scale=norm_scale, x=x)
    if norm_scale != norm_scale:
        # Update returns with the point untouched (point.cc:74-75); HasConverged still runs (map.cc:491)
        if has_converged(st["sigma2"], st["rho"], st["cos_alpha"], st["last_distance"]):
            pos = position(st["rho"])
            out.update(outcome=FIXED_STALE, cos_alpha=st["cos_alpha"], last_distance=st["last_distance"], position=pos)
            out["row"] = dict(P=pos, fixed=1)
        return out
    sigma2, rho, a, b, z_range = st["sigma2"], st["rho"], st["a"], st["b"], st["z_range"]
    s2 = 1. / (1. / sigma2 + _div(1., tau2))
    m = s2 * (rho / sigma2 + _div(x, tau2))
    C1 = a / (a + b) * pdf_normal(rho, norm_scale, x, pi, ulps[4])
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
    pos = position(rho if fault == "position_old_rho" else rho_new)
    cos_alpha = parallax(ref_world[4:7], cur_world[4:7], pos)                # point.cc:97
    last_distance = norm3((cur_world[4] - pos[0], cur_world[5] - pos[1], cur_world[6] - pos[2]))   # Frame::DistanceTo, frame.h:133-136
    n_failed = st["n_failed"] if fault == "n_failed_kept" else 0
    conv = has_converged(sigma2_new, rho_new, st["cos_alpha"] if fault == "converge_prev_cos" else cos_alpha, last_distance)
    out.update(outcome=CONVERGED if conv else UPDATED, n_failed=n_failed, rho=rho_new, sigma2=sigma2_new, a=a_new, b=b_new,
               cos_alpha=cos_alpha, last_distance=last_distance, position=pos)
    out["row"] = dict(P=pos, idepth=rho_new, idepth_std=sigma2_new if fault == "row_std_sigma2" else math.sqrt(sigma2_new), n_failed=n_failed)
    if conv or fault == "row_fixed_on_updated":
        out["row"]["fixed"] = 1
    return out


# ------------------------------------------------------------------------------------------------ what a comparison may allow
N_ULP = 4            # how far the device library's acos / sin / exp may be from libm's, in ulp: an assumption (see tolerance)
MARGIN = 4.0         # over the corner combinations: interactions they miss
FLOOR_ULP = 8        # of the value itself
VALUES = ("rho", "sigma2", "a", "b", "cos_alpha", "last_distance")


def _numbers(o):
    """the float outputs of a result, by name (position as three)"""
    d = {k: o[k] for k in VALUES if o[k] is not None}
    if o["position"] is not None:
        d.update({"position%d" % i: o["position"][i] for i in range(3)})
    for k, v in o["row"].items():
        if k == "P":
            d.update({"row.P%d" % i: v[i] for i in range(3)})
        elif k in ("idepth", "idepth_std"):
            d["row." + k] = v
    return d


def spread(n_ulp=N_ULP, **kw):
    """the restatement against itself with every transcendental result moved by +-n_ulp, all 32 sign combinations ->
    (the unmoved result, per float output the largest deviation, per traced deciding quantity the largest deviation, the set of
    outcomes met)"""
    base = restate(**kw)
    b_num = _numbers(base)
    dev = dict.fromkeys(b_num, 0.0)
    tdev = {k: 0.0 for k, v in base["trace"].items() if isinstance(v, float)}
    outcomes = {base["outcome"]}
    if base["outcome"] in (UPDATED, CONVERGED):
        for bits in range(32):
            ul = tuple(n_ulp if bits >> j & 1 else -n_ulp for j in range(5))
            o = restate(ulps=ul, **kw)
            outcomes.add(o["outcome"])
            for k, v in _numbers(o).items():
                if k in dev:
                    dev[k] = max(dev[k], abs(v - b_num[k]))
            for k in tdev:
                v = o["trace"].get(k)
                if isinstance(v, float) and v == v and base["trace"][k] == base["trace"][k]:
                    tdev[k] = max(tdev[k], abs(v - base["trace"][k]))
    return base, dev, tdev, outcomes


def tolerance(n_ulp=N_ULP, **kw):
    """-> (the unmoved result, per float output the bound on |device - restatement|): MARGIN times the largest deviation over the 32
    corner combinations of +-n_ulp, plus FLOOR_ULP ulp of the value.  An output with no transcendental behind it (a miss, the position
    of a fixed point and what is computed from it) has deviation 0 and keeps the floor alone.

    n_ulp: the ROCm documentation of the device library's double-precision accuracy is not part of the tree or of the toolchain
    installed beside it, so N_ULP = 4 is an assumption: OpenCL's limits for the same library's functions are 4 ulp for acos and sin
    and 3 ulp for exp in double precision, and libm itself is within 1."""
    base, dev, _, _ = spread(n_ulp, **kw)
    return base, {k: MARGIN * dev[k] + FLOOR_ULP * math.ulp(v) if v == v and not math.isinf(v) else 0.0 for k, v in _numbers(base).items()}
