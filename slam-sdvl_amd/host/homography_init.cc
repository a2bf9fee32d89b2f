// homography_init.cc — see homography_init.h.  Line numbers name the reference's homography_init.cc unless said otherwise.
#include "homography_init.h"
#include "sdvl_host.h"

#include <float.h>
#include <math.h>

#include <algorithm>
#include <iostream>

namespace sdvl {

namespace {

inline double Det3(const double *m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

inline void Mul3(const double *a, const double *b, double *c) {  // c = a b
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

inline void MulVec3(const double *a, const double *v, double *out) {
  for (int i = 0; i < 3; i++) out[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}

inline void MulTVec3(const double *a, const double *v, double *out) {  // a^T v
  for (int i = 0; i < 3; i++) out[i] = a[i] * v[0] + a[3 + i] * v[1] + a[6 + i] * v[2];
}

inline double Dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// extra/utils.cc:133-159
void Triangulate(const double *R, const double *T, const double *vector1, const double *vector2, double *res) {
  double v2[3];
  MulVec3(R, vector2, v2);
  const double *v1 = vector1;
  const double b0 = Dot3(T, v1), b1 = Dot3(T, v2);
  const double a00 = Dot3(v1, v1), a10 = Dot3(v1, v2), a01 = -a10, a11 = -Dot3(v2, v2);
  const double det = a00 * a11 - a01 * a10;
  const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (-a10 * b0 + a00 * b1) / det;
  for (int c = 0; c < 3; c++) res[c] = (l0 * v1[c] + (T[c] + l1 * v2[c])) / 2;
}

// the normalisation of cv::findHomography's runKernel: centroid and 1 / mean absolute deviation per axis
void HartleyNorm(const std::vector<double> &p, const int32_t *idx, int n, double *c, double *s) {
  c[0] = c[1] = 0.0;
  for (int k = 0; k < n; k++) {
    c[0] += p[2 * idx[k]];
    c[1] += p[2 * idx[k] + 1];
  }
  c[0] /= n;
  c[1] /= n;
  double a[2] = {0.0, 0.0};
  for (int k = 0; k < n; k++) {
    a[0] += fabs(p[2 * idx[k]] - c[0]);
    a[1] += fabs(p[2 * idx[k] + 1] - c[1]);
  }
  for (int d = 0; d < 2; d++) {
    a[d] /= n;
    s[d] = 1.0 / (a[d] > DBL_EPSILON ? a[d] : 1.0);
  }
}

}  // namespace

void JacobiEigenSym(int n, double *A, double *V, double *eig) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[n * i + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 100; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) (i == j ? diag : off) += A[n * i + j] * A[n * i + j];
    if (off <= 1e-32 * diag || off == 0.0) break;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = A[n * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[n * q + q] - A[n * p + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {  // columns p, q
          const double akp = A[n * k + p], akq = A[n * k + q];
          A[n * k + p] = c * akp - s * akq;
          A[n * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {  // rows p, q
          const double apk = A[n * p + k], aqk = A[n * q + k];
          A[n * p + k] = c * apk - s * aqk;
          A[n * q + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double vkp = V[n * k + p], vkq = V[n * k + q];
          V[n * k + p] = c * vkp - s * vkq;
          V[n * k + q] = s * vkp + c * vkq;
        }
      }
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[n * a + a] < A[n * b + b]; });
  std::vector<double> Vs(static_cast<size_t>(n) * n);
  for (int j = 0; j < n; j++) {
    eig[j] = A[n * order[j] + order[j]];
    for (int k = 0; k < n; k++) Vs[n * k + j] = V[n * k + order[j]];
  }
  std::copy(Vs.begin(), Vs.end(), V);
}

void JacobiSvd3(const double A[9], double U[9], double s[3], double V[9]) {
  double B[9], Vasc[9], eig[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) B[3 * i + j] = A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j];  // A^T A
  JacobiEigenSym(3, B, Vasc, eig);
  for (int j = 0; j < 3; j++) {  // descending
    s[j] = sqrt(std::max(eig[2 - j], 0.0));
    for (int k = 0; k < 3; k++) V[3 * k + j] = Vasc[3 * k + (2 - j)];
  }
  for (int j = 0; j < 2; j++) {  // u_j = A v_j / s_j
    const double v[3] = {V[j], V[3 + j], V[6 + j]};
    double u[3];
    MulVec3(A, v, u);
    const double norm = sqrt(Dot3(u, u));
    for (int k = 0; k < 3; k++) U[3 * k + j] = u[k] / norm;
  }
  {  // the third column: A v_3 when it has a direction, completed to an orthogonal matrix either way
    const double u0[3] = {U[0], U[3], U[6]}, u1[3] = {U[1], U[4], U[7]};
    double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
    const double v[3] = {V[2], V[5], V[8]};
    double av[3];
    MulVec3(A, v, av);
    if (Dot3(av, u2) < 0)
      for (int k = 0; k < 3; k++) u2[k] = -u2[k];
    for (int k = 0; k < 3; k++) U[3 * k + 2] = u2[k];
  }
}

HomographyMath::HomographyMath(const double cam[4], double inlier_error_threshold, double map_scale)
    : fx_(cam[0]), fy_(cam[1]), u0_(cam[2]), v0_(cam[3]), thr_(inlier_error_threshold), map_scale_(map_scale) {
  for (int i = 0; i < 9; i++) bestH_[i] = R_[i] = 0.0;
  t_[0] = t_[1] = t_[2] = 0.0;
}

void HomographyMath::SetTracks(int n, const float *pixels1, const float *pixels2) {
  n_ = n;
  vectors1_.resize(3 * static_cast<size_t>(n));
  vectors2_.resize(3 * static_cast<size_t>(n));
  src_.resize(2 * static_cast<size_t>(n));
  dst_.resize(2 * static_cast<size_t>(n));
  for (int i = 0; i < n; i++) {
    const float *px[2] = {pixels1 + 2 * i, pixels2 + 2 * i};
    double *vec[2] = {&vectors1_[3 * i], &vectors2_[3 * i]};
    double *out[2] = {&src_[2 * i], &dst_[2 * i]};
    for (int f = 0; f < 2; f++) {
      // Camera::Unproject (camera.h): the unit ray of the pixel (:69-71 through Feature, :213-215)
      const double x = (static_cast<double>(px[f][0]) - u0_) / fx_, y = (static_cast<double>(px[f][1]) - v0_) / fy_;
      const double norm = sqrt(x * x + y * y + 1.0);
      vec[f][0] = x / norm;
      vec[f][1] = y / norm;
      vec[f][2] = 1.0 / norm;
      // :246-249: Camera::SimpleProject, then cv::Point2f — the correspondences are rounded to float (kept)
      out[f][0] = static_cast<double>(static_cast<float>(vec[f][0] / vec[f][2]));
      out[f][1] = static_cast<double>(static_cast<float>(vec[f][1] / vec[f][2]));
    }
  }
}

// :237-282 from the cv::findHomography call on: the RANSAC ran on the device, its refit on the inliers is done here
bool HomographyMath::ComputeHomography(int n_ransac_inliers, const int32_t *ransac_inliers, int min_init_corners) {
  inliers_.clear();
  triangulations_.clear();
  decompositions_.clear();
  if (n_ransac_inliers < 4 || !ransac_inliers) return false;
  for (int k = 0; k < n_ransac_inliers; k++)
    if (ransac_inliers[k] < 0 || ransac_inliers[k] >= n_) return false;
  {  // cv::findHomography's final runKernel on the inliers (fundam.cpp): normalised DLT, smallest eigenvector of L^T L
    double cM[2], sM[2], cm[2], sm[2];
    HartleyNorm(src_, ransac_inliers, n_ransac_inliers, cM, sM);
    HartleyNorm(dst_, ransac_inliers, n_ransac_inliers, cm, sm);
    double LtL[81], V[81], eig[9];
    for (int i = 0; i < 81; i++) LtL[i] = 0.0;
    for (int k = 0; k < n_ransac_inliers; k++) {
      const int i = ransac_inliers[k];
      const double X = (src_[2 * i] - cM[0]) * sM[0], Y = (src_[2 * i + 1] - cM[1]) * sM[1];
      const double x = (dst_[2 * i] - cm[0]) * sm[0], y = (dst_[2 * i + 1] - cm[1]) * sm[1];
      const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x}, Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
      for (int a = 0; a < 9; a++)
        for (int b = 0; b < 9; b++) LtL[9 * a + b] += Lx[a] * Lx[b] + Ly[a] * Ly[b];
    }
    JacobiEigenSym(9, LtL, V, eig);
    double H0[9], tmp[9];
    for (int k = 0; k < 9; k++) H0[k] = V[9 * k];  // the eigenvector of the smallest eigenvalue
    const double inv2[9] = {1.0 / sm[0], 0, cm[0], 0, 1.0 / sm[1], cm[1], 0, 0, 1};
    const double norm1[9] = {sM[0], 0, -cM[0] * sM[0], 0, sM[1], -cM[1] * sM[1], 0, 0, 1};
    Mul3(inv2, H0, tmp);
    Mul3(tmp, norm1, bestH_);
    const double h22 = bestH_[8];
    for (int k = 0; k < 9; k++) bestH_[k] /= h22;
    // (OpenCV polishes H with Levenberg-Marquardt on the inliers here: left out)
  }
  if (!DecomposeHomography()) return false;  // :265-266
  CheckInliers();                            // :267
  n_h_inliers_ = static_cast<int>(inliers_.size());
  if (inliers_.empty() || !ChooseBestDecomposition()) return false;  // :268
  for (int k = 0; k < 9; k++) R_[k] = decompositions_[0].R[k];      // :271-272
  for (int k = 0; k < 3; k++) t_[k] = decompositions_[0].t[k];
  CheckDecompositionInliers();               // :275
  if (static_cast<int>(inliers_.size()) < min_init_corners) return false;  // :276-279
  if (triangulations_.empty()) return false;  // :102-103
  // InitSecondFrame :111-121 with frame 1 at the identity: the map is scaled so that the median depth is MapScale()
  std::vector<double> depths(n_);
  for (int i = 0; i < n_; i++) depths[i] = triangulations_[3 * i + 2];
  std::nth_element(depths.begin(), depths.begin() + depths.size() / 2, depths.end());  // GetMedianVector, extra/utils.cc:215-220
  depth_ = depths[depths.size() / 2];
  const double scale = map_scale_ / depth_;
  double centre[3], neg_t[3] = {-t_[0], -t_[1], -t_[2]};
  MulTVec3(R_, neg_t, centre);  // frame2_->GetWorldPosition()
  for (int k = 0; k < 3; k++) centre[k] = 0.0 + scale * (centre[k] - 0.0);
  double rt[3];
  MulVec3(R_, centre, rt);
  for (int k = 0; k < 3; k++) t_[k] = -rt[k];
  return true;
}

// :284-297.  The error is in normalised coordinates and the threshold InlierErrorThreshold() unscaled (pixels): every match passes.
// Kept as the reference has it.
void HomographyMath::CheckInliers() {
  inliers_.clear();
  for (int i = 0; i < n_; i++) {
    const double v[3] = {src_[2 * i], src_[2 * i + 1], 1.0};
    double p[3];
    MulVec3(bestH_, v, p);
    const double ex = dst_[2 * i] - p[0] / p[2], ey = dst_[2 * i + 1] - p[1] / p[2];
    if (sqrt(ex * ex + ey * ey) <= thr_) inliers_.push_back(i);
  }
}

// :329-443
bool HomographyMath::DecomposeHomography() {
  decompositions_.clear();
  double U[9], sv[3], V[9];
  JacobiSvd3(bestH_, U, sv, V);
  const double d1 = fabs(sv[0]), d2 = fabs(sv[1]), d3 = fabs(sv[2]);
  const double s = Det3(U) * Det3(V);
  const double dPrime_PM = d2;
  int nCase;
  if (d1 != d2 && d2 != d3) nCase = 1;
  else if (d1 == d2 && d2 == d3) nCase = 3;
  else nCase = 2;
  if (nCase != 1) return false;  // :353-356
  const double x1_PM = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const double x2 = 0;
  const double x3_PM = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const double e1[4] = {1.0, -1.0, 1.0, -1.0}, e3[4] = {1.0, 1.0, -1.0, -1.0};
  HomographyDecomposition dec;
  auto normal = [&](int signs) {
    const double np[3] = {x1_PM * e1[signs], x2, x3_PM * e3[signs]};
    MulVec3(V, np, dec.v3n);
  };
  // Case 1, d' > 0 (:379-404)
  dec.d = s * dPrime_PM;
  for (int signs = 0; signs < 4; signs++) {
    const double dSinTheta = (d1 - d3) * x1_PM * x3_PM * e1[signs] * e3[signs] / d2;
    const double dCosTheta = (d1 * x3_PM * x3_PM + d3 * x1_PM * x1_PM) / d2;
    const double Rp[9] = {dCosTheta, 0, -dSinTheta, 0, 1, 0, dSinTheta, 0, dCosTheta};
    std::copy(Rp, Rp + 9, dec.m3Rp);
    dec.v3Tp[0] = (d1 - d3) * x1_PM * e1[signs];
    dec.v3Tp[1] = 0.0;
    dec.v3Tp[2] = (d1 - d3) * -x3_PM * e3[signs];
    normal(signs);
    decompositions_.push_back(dec);
  }
  // Case 1, d' < 0 (:406-431)
  dec.d = s * -dPrime_PM;
  for (int signs = 0; signs < 4; signs++) {
    const double dSinPhi = (d1 + d3) * x1_PM * x3_PM * e1[signs] * e3[signs] / d2;
    const double dCosPhi = (d3 * x1_PM * x1_PM - d1 * x3_PM * x3_PM) / d2;
    const double Rp[9] = {dCosPhi, 0, dSinPhi, 0, -1, 0, dSinPhi, 0, -dCosPhi};
    std::copy(Rp, Rp + 9, dec.m3Rp);
    dec.v3Tp[0] = (d1 + d3) * x1_PM * e1[signs];
    dec.v3Tp[1] = 0.0;
    dec.v3Tp[2] = (d1 + d3) * x3_PM * e3[signs];
    normal(signs);
    decompositions_.push_back(dec);
  }
  // :433-440: R = s U R' V^T, t = U t'
  double Vt[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
  for (HomographyDecomposition &d : decompositions_) {
    double a[9], b[9];
    Mul3(U, d.m3Rp, a);
    Mul3(a, Vt, b);
    for (int k = 0; k < 9; k++) d.R[k] = s * b[k];
    MulVec3(U, d.v3Tp, d.t);
  }
  return true;
}

// :449-533.  std::sort on the score alone in the reference; a stable sort here, so that equal scores keep their order on every library
bool HomographyMath::ChooseBestDecomposition() {
  auto by_score = [](const HomographyDecomposition &a, const HomographyDecomposition &b) { return a.score < b.score; };
  for (HomographyDecomposition &decom : decompositions_) {  // :455-469: 8 -> 4
    int nPositive = 0;
    for (int i : inliers_) {
      const double dVisibilityTest = (bestH_[6] * src_[2 * i] + bestH_[7] * src_[2 * i + 1] + bestH_[8]) / decom.d;
      if (dVisibilityTest > 0.0) nPositive++;
    }
    decom.score = -nPositive;
  }
  std::stable_sort(decompositions_.begin(), decompositions_.end(), by_score);
  decompositions_.resize(4);
  for (HomographyDecomposition &decom : decompositions_) {  // :471-486: 4 -> 2
    int nPositive = 0;
    for (int i : inliers_) {
      const double v3[3] = {src_[2 * i], src_[2 * i + 1], 1.0};
      if (Dot3(v3, decom.v3n) / decom.d > 0.0) nPositive++;
    }
    decom.score = -nPositive;
  }
  std::stable_sort(decompositions_.begin(), decompositions_.end(), by_score);
  decompositions_.resize(2);
  scores_[0] = -decompositions_[0].score;
  scores_[1] = -decompositions_[1].score;
  const double dRatio = static_cast<double>(decompositions_[1].score) / static_cast<double>(decompositions_[0].score);
  if (dRatio < 0.9) {  // no ambiguity (:492-493)
    decompositions_.erase(decompositions_.begin() + 1);
  } else {             // two-way ambiguity: the Sampson score of all points (:494-530)
    const double dErrorSquaredLimit = thr_ * thr_ * 4;
    double adSampsonusScores[2];
    for (int i = 0; i < 2; i++) {
      const double *R = decompositions_[i].R, *t = decompositions_[i].t;
      double E[9];
      for (int j = 0; j < 3; j++) {  // column j = t x (column j of R)
        const double r[3] = {R[j], R[3 + j], R[6 + j]};
        E[j] = t[1] * r[2] - t[2] * r[1];
        E[3 + j] = t[2] * r[0] - t[0] * r[2];
        E[6 + j] = t[0] * r[1] - t[1] * r[0];
      }
      double dSumError = 0;
      for (int m = 0; m < n_; m++) {
        double d = SampsonusError(E, m);
        if (d > dErrorSquaredLimit) d = dErrorSquaredLimit;
        dSumError += d;
      }
      adSampsonusScores[i] = dSumError;
    }
    if (adSampsonusScores[0] <= adSampsonusScores[1]) decompositions_.erase(decompositions_.begin() + 1);
    else decompositions_.erase(decompositions_.begin());
  }
  return true;
}

// :535-559
double HomographyMath::SampsonusError(const double E[9], int i) const {
  const double v3[3] = {src_[2 * i], src_[2 * i + 1], 1.0}, v3Dash[3] = {dst_[2 * i], dst_[2 * i + 1], 1.0};
  double fv3[3], fTv3Dash[3];
  MulVec3(E, v3, fv3);
  MulTVec3(E, v3Dash, fTv3Dash);
  const double dError = Dot3(fv3, v3Dash);
  return dError * dError / ((fv3[0] * fv3[0] + fv3[1] * fv3[1]) + (fTv3Dash[0] * fTv3Dash[0] + fTv3Dash[1] * fTv3Dash[1]));
}

// :299-327: every match triangulated from frame 2's point of view, both reprojection errors in pixels (x fx)
void HomographyMath::CheckDecompositionInliers() {
  inliers_.clear();
  triangulations_.resize(3 * static_cast<size_t>(n_));
  const double ratio = fx_;
  for (int i = 0; i < n_; i++) {
    double *xyz = &triangulations_[3 * i];
    const double *v2 = &vectors2_[3 * i], *v1 = &vectors1_[3 * i];
    Triangulate(R_, t_, v2, v1, xyz);
    // :561-564
    const double ax = v2[0] / v2[2] - xyz[0] / xyz[2], ay = v2[1] / v2[2] - xyz[1] / xyz[2];
    const double err1 = sqrt(ax * ax + ay * ay) * ratio;
    // :566-571
    const double rel[3] = {xyz[0] - t_[0], xyz[1] - t_[1], xyz[2] - t_[2]};
    double pc[3];
    MulTVec3(R_, rel, pc);
    const double bx = v1[0] / v1[2] - pc[0] / pc[2], by = v1[1] / v1[2] - pc[1] / pc[2];
    const double err2 = sqrt(bx * bx + by * by) * ratio;
    if (err1 <= thr_ && err2 <= thr_) inliers_.push_back(i);
  }
}


// ------------------------------------------------------------------------------------------------------------ HomographyInit
namespace {
const int kMinOrbThreshold = 100;  // MIN_ORB_THRESHOLD, matcher.h:37
const int kRansacMaxIts = 2000;    // cv::findHomography's maxIters
const double kRansacConfidence = 0.995;

SE3 PoseFrom(const double *R, const double *t) {  // rotation matrix (row-major) + translation -> SE3 (unit quaternion, Shepperd)
  double q[4];
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) {
    const double s = sqrt(tr + 1.0) * 2;
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double p7[7] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n, t[0], t[1], t[2]};
  return SE3::FromArray(p7);
}

// extra/utils.cc:193-205
bool DepthFromTriangulation(const SE3 &pose, const Vector3d &v_ref, const Vector3d &v_cur, double *depth) {
  const double rot7[7] = {pose.pod().q0, pose.pod().q1, pose.pod().q2, pose.pod().q3, 0, 0, 0};
  const Vector3d a0 = SE3::FromArray(rot7) * v_ref;  // R v_ref
  const double m00 = a0(0) * a0(0) + a0(1) * a0(1) + a0(2) * a0(2), m01 = a0(0) * v_cur(0) + a0(1) * v_cur(1) + a0(2) * v_cur(2);
  const double m11 = v_cur(0) * v_cur(0) + v_cur(1) * v_cur(1) + v_cur(2) * v_cur(2);
  const double det = m00 * m11 - m01 * m01;
  if (det < 0.000001) return false;
  const double i00 = m11 / det, i01 = -m01 / det;
  const Vector3d t = pose.GetTranslation();
  double d0 = 0.0;
  for (int c = 0; c < 3; c++) d0 += (-i00 * a0(c) - i01 * v_cur(c)) * t(c);
  *depth = fabs(d0);
  return true;
}

int Hamming32(const uint8_t *a, const uint8_t *b) {  // ORBDetector::Distance, extra/orb_detector.cc:398-410
  int d = 0;
  for (int k = 0; k < 32; k++) d += __builtin_popcount(static_cast<unsigned>(a[k] ^ b[k]));
  return d;
}
}  // namespace

HomographyInit::HomographyInit(Map *map, int min_shift) : map_(map), min_shift_(min_shift) {}

// :41-48
void HomographyInit::Reset() {
  pixels1_.clear();
  pixels2_.clear();
  vectors1_.clear();
  vectors2_.clear();
  frame1_ = nullptr;
  frame2_ = nullptr;
  math_.reset();
}

// :50-81
bool HomographyInit::InitFirstFrame(const std::shared_ptr<Frame> &frame) {
  frame1_ = frame;
  frame1_->FilterCorners();  // :58 (the filtered corners and their level come back from the device in FilteredCorner order)
  pixels1_.clear();
  pixels2_.clear();
  vectors1_.clear();
  const int n = frame1_->NumFiltered();
  for (int k = 0; k < n; k++) {
    const Vector3i corner = frame1_->FilteredCorner(k);
    const int scale = (1 << corner(2));
    const Vector2d pos(corner(0) * scale, corner(1) * scale);  // :69
    pixels1_.push_back(static_cast<float>(pos(0)));            // cv::Point2f, :70
    pixels1_.push_back(static_cast<float>(pos(1)));
    vectors1_.push_back(frame1_->GetCamera()->Unproject(pos)); // Feature::GetVector, :71
  }
  if (NumPixels() < Config::MinInitCorners()) return false;    // :75-76
  pixels2_ = pixels1_;  // :79: optical flow will search starting from pixels2_ values
  return true;
}

void HomographyInit::BeginSecondFrame(const std::shared_ptr<Frame> &frame, int pt_begin, sdvl_klt_job *job) {
  frame2_ = frame;  // :92
  job->prev = frame1_->device();
  job->next = frame2_->device();
  job->pt_begin = pt_begin;
  job->pt_end = pt_begin + NumPixels();
}

// TrackSecondFrame :200-234, behind the cv::calcOpticalFlowPyrLK call (sdvl_klt_track, which has written pixels2_)
bool HomographyInit::FinishTrack(const uint8_t *status) {
  Camera *camera = frame2_->GetCamera();
  const int n = NumPixels();
  std::vector<float> p1, p2;
  std::vector<Vector3d> v1;
  std::vector<double> shifts;
  vectors2_.clear();
  for (int i = 0; i < n; i++) {
    if (!status[i]) continue;  // :205-210: lost points leave all three lists
    p1.insert(p1.end(), {pixels1_[2 * i], pixels1_[2 * i + 1]});
    p2.insert(p2.end(), {pixels2_[2 * i], pixels2_[2 * i + 1]});
    v1.push_back(vectors1_[i]);
    vectors2_.push_back(camera->Unproject(Vector2d(pixels2_[2 * i], pixels2_[2 * i + 1])));  // :213-215
    const double dx = static_cast<double>(pixels1_[2 * i]) - pixels2_[2 * i], dy = static_cast<double>(pixels1_[2 * i + 1]) - pixels2_[2 * i + 1];
    shifts.push_back(sqrt(dx * dx + dy * dy));  // :218
  }
  pixels1_.swap(p1);
  pixels2_.swap(p2);
  vectors1_.swap(v1);
  if (shifts.empty()) return false;  // :225-226
  std::nth_element(shifts.begin(), shifts.begin() + shifts.size() / 2, shifts.end());  // GetMedianVector
  const double shift = shifts[shifts.size() / 2];
  return shift >= min_shift_ && NumPixels() >= Config::MinInitCorners();  // :234
}

void HomographyInit::HomographyInput(const RandStream &rng, int max_its, std::vector<double> *src, std::vector<double> *dst,
                                     std::vector<int32_t> *draws4) {
  Camera *camera = frame1_->GetCamera();
  const double cam[4] = {camera->GetFx(), camera->GetFy(), camera->GetU0(), camera->GetV0()};
  math_.reset(new HomographyMath(cam, Config::InlierErrorThreshold(), Config::MapScale()));
  math_->SetTracks(NumPixels(), pixels1_.data(), pixels2_.data());  // :243-250 (correspondences rounded to float)
  *src = math_->Src();
  *dst = math_->Dst();
  RandStream copy = rng;
  const int n = NumPixels();
  draws4->resize(4 * static_cast<size_t>(max_its));
  for (int32_t &d : *draws4) d = copy.Next() % n;
}

// ComputeHomography :254-282, then InitSecondFrame :102-182
bool HomographyInit::FinishSecondFrame(const sdvl_homography_result &res, const int32_t *ransac_inliers, RandStream *rng) {
  for (int k = 0; k < 4 * res.n_its; k++) rng->Next();  // the draws the RANSAC consumed
  if (res.best_draw < 0) return false;
  if (!math_->ComputeHomography(res.n_inliers, ransac_inliers, Config::MinInitCorners())) {
    std::cerr << "[ERROR] Homography Init: Not enough inliers" << std::endl;
    return false;
  }
  Camera *camera = frame2_->GetCamera();
  const int margin = Config::UseORB() ? 4 + Config::ORBSize() / 2 : 1 + Config::PatchSize() / 2;  // :105-109
  // :111-121: the map was rescaled inside ComputeHomography (Translation() is scaled); frame1 need not sit at the identity
  const SE3 se3 = PoseFrom(math_->Rotation(), math_->Translation());
  frame2_->SetPose(se3 * frame1_->GetPose());
  const std::vector<int> &inliers = math_->Inliers();
  const std::vector<double> &tri = math_->Triangulations();
  // descriptors of both ends of every inlier in two device calls (detector_.GetDescriptor at level 0, :141-149)
  std::vector<int32_t> xyl1, xyl2;
  std::vector<uint8_t> d1, d2;
  if (Config::UseORB() && !inliers.empty()) {
    for (int i : inliers) {
      xyl1.insert(xyl1.end(), {static_cast<int32_t>(pixels1_[2 * i]), static_cast<int32_t>(pixels1_[2 * i + 1]), 0});  // p1.cast<int>()
      xyl2.insert(xyl2.end(), {static_cast<int32_t>(pixels2_[2 * i]), static_cast<int32_t>(pixels2_[2 * i + 1]), 0});
    }
    // a position outside the descriptor's margin is skipped below before its descriptor is read; describe it at a safe place
    for (size_t k = 0; k < inliers.size(); k++)
      for (std::vector<int32_t> *v : {&xyl1, &xyl2}) {
        const Vector2i p((*v)[3 * k], (*v)[3 * k + 1]);
        if (!camera->IsInsideImage(p, margin)) { (*v)[3 * k] = margin; (*v)[3 * k + 1] = margin; }
      }
    d1.resize(32 * inliers.size());
    d2.resize(32 * inliers.size());
    Device *dev = Device::Current();
    const int m = static_cast<int>(inliers.size());
    dev->Check(sdvl_orb_describe_points(dev->ctx(), frame1_->device(), m, xyl1.data(), d1.data(), nullptr), "sdvl_orb_describe_points");
    dev->Check(sdvl_orb_describe_points(dev->ctx(), frame2_->device(), m, xyl2.data(), d2.data(), nullptr), "sdvl_orb_describe_points");
  }
  MapperMap *mapper = dynamic_cast<MapperMap *>(map_);
  int nfeatures = 0;
  const SE3 pose = frame2_->GetPose() * frame1_->GetPose().Inverse();  // :132
  for (size_t k = 0; k < inliers.size(); k++) {  // :124-175
    const int i = inliers[k];
    const Vector2d p1(pixels1_[2 * i], pixels1_[2 * i + 1]), p2(pixels2_[2 * i], pixels2_[2 * i + 1]);
    const Vector2i ip1(static_cast<int>(p1(0)), static_cast<int>(p1(1))), ip2(static_cast<int>(p2(0)), static_cast<int>(p2(1)));
    if (!camera->IsInsideImage(ip1, margin) || !camera->IsInsideImage(ip2, margin) || tri[3 * i + 2] < 0) continue;  // :128-129
    double depth = 0.0;
    if (!DepthFromTriangulation(pose, vectors1_[i], vectors2_[i], &depth)) continue;  // :133-134
    std::shared_ptr<Point> candidate = std::make_shared<Point>();
    std::shared_ptr<Feature> feature1 = std::make_shared<Feature>(frame1_, candidate, p1, vectors1_[i], 0);
    std::shared_ptr<Feature> feature2 = std::make_shared<Feature>(frame2_, candidate, p2, vectors2_[i], 0);
    if (Config::UseORB()) {  // :141-154
      feature1->SetDescriptor(&d1[32 * k]);
      feature2->SetDescriptor(&d2[32 * k]);
      if (Hamming32(&d1[32 * k], &d2[32 * k]) > kMinOrbThreshold) continue;
    }
    candidate->InitCandidate(feature1, depth);  // :157-163
    frame1_->AddFeature(feature1);
    candidate->AddFeature(feature1);
    frame2_->AddFeature(feature2);
    candidate->AddFeature(feature2);
    if (mapper) mapper->AddCandidate(candidate);  // :171 (`fixed` is false)
    nfeatures++;
  }
  frame1_->AddConnection(std::make_pair(frame2_, nfeatures));  // :178-179
  frame2_->AddConnection(std::make_pair(frame1_, nfeatures));
  return nfeatures >= Config::MinInitCorners();  // :182
}

// :83-183 for one tracker
bool HomographyInit::InitSecondFrame(const std::shared_ptr<Frame> &frame, RandStream *rng) {
  Device *dev = Device::Current();
  sdvl_klt_job job;
  BeginSecondFrame(frame, 0, &job);
  const int n = NumPixels();
  if (n == 0) return false;
  std::vector<uint8_t> status(n);
  const sdvl_klt_params kp = {30, Config::PyramidLevels() - 1, 30, 0, 0.001, 1e-4};  // :195-198
  dev->Check(sdvl_klt_track(dev->ctx(), 1, &job, n, pixels1_.data(), pixels2_.data(), status.data(), nullptr, &kp), "sdvl_klt_track");
  if (!FinishTrack(status.data())) return false;  // :96-97
  std::vector<double> src, dst;
  std::vector<int32_t> draws, inl(NumPixels());
  HomographyInput(*rng, kRansacMaxIts, &src, &dst, &draws);
  const sdvl_homography_job hj = {0, NumPixels(), 0, kRansacMaxIts};
  sdvl_homography_result res;
  dev->Check(sdvl_homography_ransac(dev->ctx(), 1, &hj, NumPixels(), src.data(), dst.data(), kRansacMaxIts, draws.data(),
                                    2. / frame1_->GetCamera()->GetFx(), kRansacMaxIts, kRansacConfidence, &res, inl.data()),
             "sdvl_homography_ransac");
  return FinishSecondFrame(res, inl.data(), rng);
}

}  // namespace sdvl
