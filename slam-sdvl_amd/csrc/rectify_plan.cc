// rectify_plan.cc — sdvl_stereo_rectify_plan: a calibrated stereo rig -> the two rotations and the one pinhole camera of its rectified
// pair (include/sdvl_hip.h states the rule; tests/rectify_restatement.py is its specification).  Plain C++ in FP64, no device: it is
// linked into libsdvl_hip.so and compiles on its own (host/rectify_plan_check.cc).  Build with -ffp-contract=off: every expression
// rounds as written, which is what lets the restatement agree to the last bits.
#include <cmath>

#include "../../include/sdvl_hip.h"

namespace {

struct Mat3 {
  double m[9];
};

Mat3 identity3() { return Mat3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }

Mat3 mul3(const Mat3 &a, const Mat3 &b) {
  Mat3 c;
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) c.m[3 * r + k] = a.m[3 * r] * b.m[k] + a.m[3 * r + 1] * b.m[3 + k] + a.m[3 * r + 2] * b.m[6 + k];
  return c;
}

Mat3 transpose3(const Mat3 &a) { return Mat3{{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}}; }

void apply3(const Mat3 &a, const double *v, double *out) {
  for (int r = 0; r < 3; r++) out[r] = a.m[3 * r] * v[0] + a.m[3 * r + 1] * v[1] + a.m[3 * r + 2] * v[2];
}

double norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// exp of a rotation vector (Rodrigues): I + sin(th) K + (1 - cos(th)) K K with K the cross-product matrix of w / th
Mat3 rotation_of(const double *w) {
  const double th = norm3(w);
  if (th < 1e-15) return identity3();
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const Mat3 K{{0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0}};
  const Mat3 KK = mul3(K, K);
  const double s = std::sin(th), c = 1 - std::cos(th);
  Mat3 R = identity3();
  for (int i = 0; i < 9; i++) R.m[i] = R.m[i] + s * K.m[i] + c * KK.m[i];
  return R;
}

// the rotation vector of R, for turns below 90 degrees: the axis from R's skew part, the angle from atan2(|skew part|, (trace - 1) / 2)
void rotation_vector_of(const Mat3 &R, double *om) {
  const double v[3] = {0.5 * (R.m[7] - R.m[5]), 0.5 * (R.m[2] - R.m[6]), 0.5 * (R.m[3] - R.m[1])};
  const double s = norm3(v), c = 0.5 * (R.m[0] + R.m[4] + R.m[8] - 1);
  if (s < 1e-15) {
    om[0] = om[1] = om[2] = 0;
    return;
  }
  const double th = std::atan2(s, c);
  for (int i = 0; i < 3; i++) om[i] = v[i] / s * th;
}

// the ray of raw pixel (u, v) without its lens: 50 fixed-point iterations of the radial-tangential model, the forward model's
// expressions in sdvl_undistort's order
void undistort_point(const sdvl_camera &K, const sdvl_distortion &D, double u, double v, double *x_out, double *y_out) {
  const double k1 = D.d[0], k2 = D.d[1], p1 = D.d[2], p2 = D.d[3], k3 = D.d[4];
  const double xd = (u - K.u0) / K.fx, yd = (v - K.v0) / K.fy;
  double x = xd, y = yd;
  for (int it = 0; it < 50; it++) {
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double dx = p1 * _2xy + p2 * (r2 + 2 * x2), dy = p1 * (r2 + 2 * y2) + p2 * _2xy;
    x = (xd - dx) / kr;
    y = (yd - dy) / kr;
  }
  *x_out = x;
  *y_out = y;
}

struct Box {
  double x0, x1, y0, y1;
};

// the inner rectangle of one camera in the rectified frame's normalised coordinates
Box inner_rectangle(const sdvl_camera &K, const sdvl_distortion &D, const Mat3 &R, int w, int h) {
  Box b{-HUGE_VAL, HUGE_VAL, -HUGE_VAL, HUGE_VAL};
  bool finite = true;
  const auto ray = [&](double u, double v, double *xr, double *yr) {
    double p[3] = {0, 0, 1}, q[3];
    undistort_point(K, D, u, v, &p[0], &p[1]);
    apply3(R, p, q);
    *xr = q[0] / q[2];
    *yr = q[1] / q[2];
    if (!(std::isfinite(*xr) && std::isfinite(*yr)) || !(q[2] > 0)) finite = false;
  };
  double x, y;
  for (int j = 0; j < w; j++) {
    ray(j, 0, &x, &y);
    b.y0 = std::fmax(b.y0, y);
    ray(j, h - 1, &x, &y);
    b.y1 = std::fmin(b.y1, y);
  }
  for (int i = 0; i < h; i++) {
    ray(0, i, &x, &y);
    b.x0 = std::fmax(b.x0, x);
    ray(w - 1, i, &x, &y);
    b.x1 = std::fmin(b.x1, x);
  }
  if (!finite) b = Box{0, 0, 0, 0};  // reads as empty
  return b;
}

bool positive(double v) { return std::isfinite(v) && v > 0; }

}  // namespace

extern "C" {

const char *sdvl_stereo_rectify_plan_message(int code) {
  switch (code) {
    case 0: return "ok";
    case SDVL_RECTIFY_PLAN_NULL: return "sdvl_stereo_rectify_plan: null rig or output";
    case SDVL_RECTIFY_PLAN_SIZE: return "sdvl_stereo_rectify_plan: image size out of range (2 .. 4095 a side)";
    case SDVL_RECTIFY_PLAN_T: return "sdvl_stereo_rectify_plan: T is zero or not finite";
    case SDVL_RECTIFY_PLAN_R: return "sdvl_stereo_rectify_plan: R is not a rotation (R^T R differs from I by more than 1e-9) or turns by more than 90 degrees";
    case SDVL_RECTIFY_PLAN_VERTICAL: return "sdvl_stereo_rectify_plan: a vertical rig (|t_y| > |t_x|); horizontal rigs only";
    case SDVL_RECTIFY_PLAN_ORDER: return "sdvl_stereo_rectify_plan: t_x > 0, the right camera stands left of the left one (X_right = R X_left + T); swap the cameras";
    case SDVL_RECTIFY_PLAN_EMPTY: return "sdvl_stereo_rectify_plan: the two cameras' inner rectangles do not intersect";
    case SDVL_RECTIFY_PLAN_INTRINSICS: return "sdvl_stereo_rectify_plan: a focal length is not finite and positive";
    default: return "sdvl_stereo_rectify_plan: unknown code";
  }
}

int sdvl_stereo_rectify_plan(const sdvl_stereo_rig *rig, int width, int height, const sdvl_camera *override_or_null, sdvl_stereo_rectified *out) {
  if (!rig || !out) return SDVL_RECTIFY_PLAN_NULL;
  if (width < 2 || height < 2 || width > 4095 || height > 4095) return SDVL_RECTIFY_PLAN_SIZE;
  if (!positive(rig->left.fx) || !positive(rig->left.fy) || !positive(rig->right.fx) || !positive(rig->right.fy)) return SDVL_RECTIFY_PLAN_INTRINSICS;
  if (override_or_null && (!positive(override_or_null->fx) || !positive(override_or_null->fy) || !std::isfinite(override_or_null->u0) ||
                           !std::isfinite(override_or_null->v0)))
    return SDVL_RECTIFY_PLAN_INTRINSICS;
  const double *T = rig->T;
  if (!(std::isfinite(T[0]) && std::isfinite(T[1]) && std::isfinite(T[2])) || norm3(T) == 0) return SDVL_RECTIFY_PLAN_T;
  Mat3 R;
  for (int i = 0; i < 9; i++) R.m[i] = rig->R[i];
  const Mat3 RtR = mul3(transpose3(R), R);
  for (int i = 0; i < 9; i++)
    if (!(std::fabs(RtR.m[i] - (i % 4 == 0 ? 1.0 : 0.0)) <= 1e-9)) return SDVL_RECTIFY_PLAN_R;
  if (!(R.m[0] + R.m[4] + R.m[8] - 1 > 0)) return SDVL_RECTIFY_PLAN_R;  // cos of the turn

  // ---- the rotations
  double om[3], t[3];
  rotation_vector_of(R, om);
  const double half[3] = {-0.5 * om[0], -0.5 * om[1], -0.5 * om[2]};
  const Mat3 rr = rotation_of(half);
  apply3(rr, T, t);
  if (std::fabs(t[1]) > std::fabs(t[0])) return SDVL_RECTIFY_PLAN_VERTICAL;
  if (t[0] > 0) return SDVL_RECTIFY_PLAN_ORDER;
  const double u[3] = {t[0] > 0 ? 1.0 : -1.0, 0, 0};
  double ww[3] = {t[1] * u[2] - t[2] * u[1], t[2] * u[0] - t[0] * u[2], t[0] * u[1] - t[1] * u[0]};
  const double nw = norm3(ww);
  if (nw > 0) {
    const double tu = t[0] * u[0] + t[1] * u[1] + t[2] * u[2];
    const double angle = std::acos(std::fmin(std::fabs(tu) / norm3(t), 1.0));
    for (int i = 0; i < 3; i++) ww[i] = ww[i] * (angle / nw);
  }
  const Mat3 wR = rotation_of(ww);
  const Mat3 R1 = mul3(wR, transpose3(rr)), R2 = mul3(wR, rr);

  // ---- the rectified camera
  sdvl_camera rect;
  rect.width = width;
  rect.height = height;
  if (override_or_null) {
    rect.fx = override_or_null->fx;
    rect.fy = override_or_null->fy;
    rect.u0 = override_or_null->u0;
    rect.v0 = override_or_null->v0;
  } else {
    const Box a = inner_rectangle(rig->left, rig->left_dist, R1, width, height);
    const Box b = inner_rectangle(rig->right, rig->right_dist, R2, width, height);
    const double x0 = std::fmax(a.x0, b.x0), x1 = std::fmin(a.x1, b.x1), y0 = std::fmax(a.y0, b.y0), y1 = std::fmin(a.y1, b.y1);
    if (!(x1 > x0) || !(y1 > y0) || !std::isfinite(x1 - x0) || !std::isfinite(y1 - y0)) return SDVL_RECTIFY_PLAN_EMPTY;
    const double f = std::fmax((width - 1 + 4) / (x1 - x0), (height - 1 + 4) / (y1 - y0));
    if (!positive(f)) return SDVL_RECTIFY_PLAN_EMPTY;
    rect.fx = rect.fy = f;
    rect.u0 = (width - 1) / 2.0 - f * ((x0 + x1) / 2);
    rect.v0 = (height - 1) / 2.0 - f * ((y0 + y1) / 2);
  }
  out->left.raw = rig->left;
  out->left.dist = rig->left_dist;
  out->right.raw = rig->right;
  out->right.dist = rig->right_dist;
  for (int i = 0; i < 9; i++) {
    out->left.R[i] = R1.m[i];
    out->right.R[i] = R2.m[i];
  }
  out->left.rect = out->right.rect = rect;
  out->baseline = norm3(T);
  return 0;
}

}  // extern "C"
