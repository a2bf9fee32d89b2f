// sdvl_depth_filter.h — the arithmetic of the mapper's depth filter, stated once for the kernels (sdvl_depth_filter.hip), the host path
// (host/mapper.cc) and a host program of the tests (tests/depth_filter_math_check.cc): the loop body of Map::UpdateCandidates behind
// SearchPoint (map.cc:454-497) and what it calls.  Host and device build it with -ffp-contract=off: the same expressions, so the same
// bits up to the math library's acos / sin / exp.  Every expression stands as the reference writes it; do not rearrange one.
#ifndef SDVL_DEPTH_FILTER_H_
#define SDVL_DEPTH_FILTER_H_

#include "../../include/sdvl_hip.h"
#include "sdvl_math.h"

namespace sdvl {

// extra/utils.cc:193-205: A = [R v_ref | v_cur], depth2 = -(A^T A)^-1 A^T t, |depth2[0]|
SDVL_HD bool depth_from_triangulation(const Rigid &pose, V3 v_ref, V3 v_cur, double *depth) {
  const M3 R = se3_rot(pose);
  const V3 a0 = mvec(R, v_ref);
  const V3 a1 = v_cur;
  const double m00 = vdot(a0, a0), m01 = vdot(a0, a1), m11 = vdot(a1, a1);
  const double det = m00 * m11 - m01 * m01;
  if (det < 0.000001) return false;
  const double invdet = 1.0 / det;
  const double i00 = m11 * invdet, i01 = -m01 * invdet;
  const double n00 = -i00, n01 = -i01;
  const double r0x = n00 * a0.x + n01 * a1.x, r0y = n00 * a0.y + n01 * a1.y, r0z = n00 * a0.z + n01 * a1.z;
  const double d0 = r0x * pose.t.x + r0y * pose.t.y + r0z * pose.t.z;
  *depth = fabs(d0);
  return true;
}

// extra/utils.cc:207-213
SDVL_HD double parallax_of(V3 src1, V3 src2, V3 p3d) {
  V3 v1 = vsub(src1, p3d), v2 = vsub(src2, p3d);
  const double n1 = vnorm(v1), n2 = vnorm(v2);
  v1 = {v1.x / n1, v1.y / n1, v1.z / n1};
  v2 = {v2.x / n2, v2.y / n2, v2.z / n2};
  return vdot(v1, v2);
}

// Point::ComputeTau, point.cc:189-201
SDVL_HD double compute_tau(const Rigid &pose, V3 v, double depth, double px_error_angle) {
  const double PI = 3.14159265;
  const V3 t = pose.t;
  const V3 a = {v.x * depth - t.x, v.y * depth - t.y, v.z * depth - t.z};
  const double t_norm = vnorm(t), a_norm = vnorm(a);
  const double alpha = acos((v.x * t.x + v.y * t.y + v.z * t.z) / t_norm);
  const double beta = acos((a.x * -t.x + a.y * -t.y + a.z * -t.z) / (t_norm * a_norm));
  const double beta_plus = beta + px_error_angle;
  const double gamma_plus = PI - alpha - beta_plus;
  const double depth_plus = t_norm * sin(beta_plus) / sin(gamma_plus);
  return depth_plus - depth;
}

// Point::PDFNormal, point.cc:203-217
SDVL_HD double pdf_normal(double mean, double sd, double x) {
  const double PI = 3.14159265;
  double result = 0.0;
  if (sd <= 0) return result;
  double exponent = x - mean;
  exponent *= -exponent;
  exponent /= 2 * sd * sd;
  result = exp(exponent);
  result /= sd * sqrt(2.0 * PI);
  return result;
}

// point.cc:69: the deviation of the inverse depth for a depth and its deviation tau
SDVL_HD double tau_inverse(double depth, double tau) { return 0.5 * (1.0 / fmax(0.0000001, depth - tau) - 1.0 / (depth + tau)); }

// The Gaussian x uniform posterior of Point::Update (point.cc:70-92) for the measurement x = 1 / depth with the deviation tau_inv.
// -> false, *q untouched: norm_scale is NaN (point.cc:76).  (q apart from p on purpose: a kernel that let the update write into the
// record it returns kept those four values live across both branches and lost a wave of occupancy)
struct DepthPosterior {
  double rho, sigma2, a, b;
};
SDVL_HD bool posterior_update(const DepthPosterior &p, double z_range, double x, double tau_inv, DepthPosterior *q) {
  const double rho_ = p.rho, sigma2_ = p.sigma2, a_ = p.a, b_ = p.b;
  const double tau2 = tau_inv * tau_inv;
  const double norm_scale = sqrt(sigma2_ + tau2);
  if (norm_scale != norm_scale) return false;
  const double s2 = 1. / (1. / sigma2_ + 1. / tau2);
  const double m = s2 * (rho_ / sigma2_ + x / tau2);
  double C1 = a_ / (a_ + b_) * pdf_normal(rho_, norm_scale, x);
  double C2 = b_ / (a_ + b_) * 1. / z_range;
  const double normalization_constant = C1 + C2;
  C1 /= normalization_constant;
  C2 /= normalization_constant;
  const double f = C1 * (a_ + 1.) / (a_ + b_ + 1.) + C2 * a_ / (a_ + b_ + 1.);
  const double e = C1 * (a_ + 1.) * (a_ + 2.) / ((a_ + b_ + 1.) * (a_ + b_ + 2.)) + C2 * a_ * (a_ + 1.0) / ((a_ + b_ + 1.0) * (a_ + b_ + 2.0));
  const double rho_new = C1 * m + C2 * rho_;
  q->sigma2 = C1 * (s2 + m * m) + C2 * (sigma2_ + rho_ * rho_) - rho_new * rho_new;
  q->rho = rho_new;
  q->a = (e - f) / (f - e / f);
  q->b = q->a * (1.0 - f) / f;
  return true;
}

// Point::HasConverged, point.cc:164-178
SDVL_HD bool has_converged(bool fixed, double rho, double sigma2, double cos_alpha, double last_distance) {
  const double std_d = sqrt(sigma2) / (rho * rho);
  const double l = 4 * std_d * cos_alpha / last_distance;
  return fixed || l < 0.1;
}

// Point::GetPosition (point.cc:128-142): a fixed point's own position, a candidate's first ray at its inverse depth
SDVL_HD V3 filter_position(const sdvl_depth_state &st, const Rigid &ref_world, V3 fv, double rho) {
  const double sc = 1.0 / rho;
  return st.fixed ? V3{st.position[0], st.position[1], st.position[2]} : se3_apply(ref_world, {sc * fv.x, sc * fv.y, sc * fv.z});
}

// The loop body for one candidate.  cur7, ref7: the world -> camera poses of the current frame and of the candidate's keyframe; bearing3: its
// first observation's ray; found, px2: what the search returned.  A miss is Point::Unpromote (point.cc:109-118).  A hit: triangulation,
// the parallax of the triangulated point, the two minimum-depth tests, Point::Update (point.cc:64-100) and Point::HasConverged.
// measured (a depth camera; tests/depth_measure_restatement.py is the specification): the sample z_c, carried along the found pixel's
// ray and into the reference frame, gives the range along the candidate's ray; that range goes through the two minimum-depth tests,
// Update and HasConverged with tau = noise_abs + noise_quad z_c^2 in ComputeTau's place — no triangulation is made, so neither it nor
// the parallax test that guards it applies.  -> the point's new state; what a row of the tracking tables receives is all in it
SDVL_HD sdvl_depth_out depth_filter_item(const double *cur7, const double *ref7, const double *bearing3, bool found, const double *px2,
                                         const sdvl_depth_state &st, const Cam &cam, const sdvl_depth_params &fp, bool measured = false,
                                         double z_c = 0.0, double noise_abs = 0.0, double noise_quad = 0.0) {
  sdvl_depth_out o;
  o.outcome = SDVL_DEPTH_SKIPPED;
  o.n_failed = st.n_failed;
  o.rho = st.rho; o.sigma2 = st.sigma2; o.a = st.a; o.b = st.b;
  o.cos_alpha = 0.0; o.last_distance = 0.0;
  o.position[0] = o.position[1] = o.position[2] = 0.0;
  if (!found) {
    o.n_failed = st.n_failed + 1;
    o.b = st.b + 1.0;
    o.outcome = SDVL_DEPTH_NOT_FOUND | (o.n_failed > fp.max_failed ? SDVL_DEPTH_DELETED : 0);
    return o;
  }
  const Rigid cur = se3_from7(cur7), ref = se3_from7(ref7);
  const V3 fv = {bearing3[0], bearing3[1], bearing3[2]};
  const V3 v3d = cam_unproject(cam, {px2[0], px2[1]});
  double depth = 0.0, tau = 0.0;
  bool go = false;
  // (the triangulation stands in front of the world poses on purpose: the other order costs the kernel 26 VGPRs and a wave of occupancy)
  if (!measured) go = depth_from_triangulation(se3_mul(cur, se3_inverse(ref)), fv, v3d, &depth);  // map.cc:459
  const Rigid ref_world = se3_inverse(ref), cur_world = se3_inverse(cur);                         // Frame::GetWorldPose
  if (measured) {
    const double k = z_c / v3d.z;
    const V3 p_r = se3_apply(se3_mul(ref, se3_inverse(cur)), {v3d.x * k, v3d.y * k, v3d.z * k});
    depth = vdot(p_r, fv);  // the range along the candidate's ray
    go = depth > 0.0;
    tau = noise_abs + noise_quad * (z_c * z_c);
  } else if (go) {
    const V3 p3d = se3_apply(ref_world, {depth * fv.x, depth * fv.y, depth * fv.z});
    const double cos_alpha = parallax_of(ref_world.t, cur_world.t, p3d);
    if (cos_alpha >= 0.999999) go = false;
  }
  if (go && (depth < fp.min_depth || depth < st.depth_mean * fp.scale_min_dist)) go = false;
  if (!go) return o;
  if (!measured) tau = compute_tau(se3_mul(ref, se3_inverse(cur)), fv, depth, fp.px_error_angle);
  const double x = 1. / depth;
  DepthPosterior q;
  if (!posterior_update({st.rho, st.sigma2, st.a, st.b}, st.z_range, x, tau_inverse(depth, tau), &q)) {
    // Update returns with the point untouched; HasConverged still runs, on the old estimate
    if (has_converged(st.fixed, st.rho, st.sigma2, st.cos_alpha, st.last_distance)) {
      const V3 pos = filter_position(st, ref_world, fv, st.rho);
      o.position[0] = pos.x; o.position[1] = pos.y; o.position[2] = pos.z;
      o.cos_alpha = st.cos_alpha; o.last_distance = st.last_distance;
      o.outcome = SDVL_DEPTH_FIXED_STALE;
    }
    return o;
  }
  o.rho = q.rho; o.sigma2 = q.sigma2; o.a = q.a; o.b = q.b;
  const V3 pos = filter_position(st, ref_world, fv, o.rho);
  o.cos_alpha = parallax_of(ref_world.t, cur_world.t, pos);
  o.last_distance = vnorm(vsub(cur_world.t, pos));  // Frame::DistanceTo, frame.h:133-136
  o.n_failed = 0;
  o.position[0] = pos.x; o.position[1] = pos.y; o.position[2] = pos.z;
  o.outcome = has_converged(st.fixed, o.rho, o.sigma2, o.cos_alpha, o.last_distance) ? SDVL_DEPTH_CONVERGED : SDVL_DEPTH_UPDATED;
  return o;
}

}  // namespace sdvl

#endif  // SDVL_DEPTH_FILTER_H_
