// homography_init.h — the reference's HomographyInit (homography_init.h:34-99, homography_init.cc): the two-frame initialisation.
// HomographyInit keeps the reference's public members (InitFirstFrame, InitSecondFrame, Reset, HasError) on Frame / Map objects; its two
// OpenCV calls run on the device (sdvl_klt_track, sdvl_homography_ransac), and InitSecondFrame is also offered in phases so that a step
// runs the KLT of ALL its initialising trackers in one call and their RANSACs in another (SDVLBatch::InitializeTrackers).
// HomographyMath is its arithmetic on plain arrays: ComputeHomography, CheckInliers, DecomposeHomography, ChooseBestDecomposition,
// CheckDecompositionInliers and the map scaling of InitSecondFrame (:111-121), statement by statement.  No Eigen and no OpenCV here: the
// DLT refit of H on the RANSAC inliers and the 3x3 SVD are small Jacobi routines; OpenCV's Levenberg-Marquardt polish of H is left
// out.  Part of the reference-side file set (standalone.cc, mapper.cc; batch.cc calls it for a batch), not of frontend.cc.
#ifndef SDVL_HOMOGRAPHY_INIT_H_
#define SDVL_HOMOGRAPHY_INIT_H_

#include <stdint.h>

#include <memory>
#include <vector>

#include "frontend.h"

namespace sdvl {

// homography_init.h:34-45
struct HomographyDecomposition {
  double v3Tp[3];
  double m3Rp[9];
  double d;
  double v3n[3];
  double R[9], t[3];  // se3: frame 1 -> frame 2
  int score;
};

class HomographyMath {
 public:
  // cam = fx fy u0 v0; inlier_error_threshold = Config::InlierErrorThreshold(); map_scale = Config::MapScale()
  HomographyMath(const double cam[4], double inlier_error_threshold, double map_scale);
  // pixels1_ / pixels2_ as TrackSecondFrame leaves them (cv::Point2f: float; lost points dropped), vectors1_ / vectors2_ from them
  void SetTracks(int n, const float *pixels1, const float *pixels2);
  // src_pts / dst_pts of ComputeHomography (:243-250): Camera::SimpleProject of the vectors ROUNDED TO FLOAT (cv::Point2f), [n][2]:
  // what goes to sdvl_homography_ransac with the threshold 2 / fx (:253)
  const std::vector<double> &Src() const { return src_; }
  const std::vector<double> &Dst() const { return dst_; }
  // ComputeHomography from :253 on, given the RANSAC's inliers: refit, decomposition, choice, CheckDecompositionInliers, scaling.
  // false: degenerate motion case (:353-356), fewer than min_init_corners inliers (:276-279) or no triangulation
  bool ComputeHomography(int n_ransac_inliers, const int32_t *ransac_inliers, int min_init_corners);

  const double *BestH() const { return bestH_; }
  const double *Rotation() const { return R_; }        // se3_, frame 1 -> frame 2
  const double *Vectors1() const { return vectors1_.data(); }
  const double *Vectors2() const { return vectors2_.data(); }
  const double *Translation() const { return t_; }     // scaled to the map (InitSecondFrame :111-121)
  const std::vector<int> &Inliers() const { return inliers_; }
  const std::vector<double> &Triangulations() const { return triangulations_; }  // [n][3], frame 2's point of view (:315)
  int VisibilityScore(int k) const { return scores_[k]; }  // of the two decompositions that survive the second round
  int NumHomographyInliers() const { return n_h_inliers_; }
  double MedianDepth() const { return depth_; }

 private:
  bool DecomposeHomography();                            // :329-443
  void CheckInliers();                                   // :284-297
  bool ChooseBestDecomposition();                        // :449-533
  void CheckDecompositionInliers();                      // :299-327
  double SampsonusError(const double E[9], int i) const; // :535-559
  double fx_, fy_, u0_, v0_, thr_, map_scale_;
  int n_ = 0;
  std::vector<double> vectors1_, vectors2_;              // [n][3]
  std::vector<double> src_, dst_;                        // [n][2]
  double bestH_[9];
  std::vector<int> inliers_;
  std::vector<HomographyDecomposition> decompositions_;
  std::vector<double> triangulations_;
  double R_[9], t_[3], depth_ = 0.0;
  int scores_[2] = {0, 0}, n_h_inliers_ = 0;
};

class MapperMap;

// homography_init.h:47-99
class HomographyInit {
 public:
  HomographyInit(Map *map, int min_shift);
  ~HomographyInit() {}
  bool InitFirstFrame(const std::shared_ptr<Frame> &frame);   // :50-81
  // :83-183 for one tracker: the phases below with one job per device call; rng: the stream the RANSAC draws from
  bool InitSecondFrame(const std::shared_ptr<Frame> &frame, RandStream *rng);
  void Reset();                                               // :41-48
  inline bool HasError() { return pixels1_.empty(); }         // homography_init.h:58

  // ---- InitSecondFrame in phases, for a step that initialises several trackers
  // frame2_ = frame; the KLT job of TrackSecondFrame (:195-198) over points [pt_begin, pt_begin + NumPixels()) of the call
  void BeginSecondFrame(const std::shared_ptr<Frame> &frame, int pt_begin, sdvl_klt_job *job);
  int NumPixels() const { return static_cast<int>(pixels1_.size() / 2); }
  const float *Pixels1() const { return pixels1_.data(); }
  float *Pixels2() { return pixels2_.data(); }                // initial flow in, result out (OPTFLOW_USE_INITIAL_FLOW)
  bool FinishTrack(const uint8_t *status);                    // TrackSecondFrame :200-234
  // src / dst of ComputeHomography (:243-250) and max_its 4-subsets from a COPY of rng (the stream itself is advanced by
  // FinishSecondFrame, by the draws the RANSAC consumed)
  void HomographyInput(const RandStream &rng, int max_its, std::vector<double> *src, std::vector<double> *dst, std::vector<int32_t> *draws4);
  // ComputeHomography from :254 on and InitSecondFrame :102-182
  bool FinishSecondFrame(const sdvl_homography_result &res, const int32_t *ransac_inliers, RandStream *rng);
  const HomographyMath *Math() const { return math_.get(); }

 private:
  Map *map_;
  std::shared_ptr<Frame> frame1_, frame2_;
  std::vector<float> pixels1_, pixels2_;                      // cv::Point2f pairs
  std::vector<Vector3d> vectors1_, vectors2_;
  int min_shift_;
  std::unique_ptr<HomographyMath> math_;
};

// the two Jacobi routines, exposed for the tests
// eigenvalues (ascending) and eigenvectors (columns of V, row-major n x n) of a symmetric matrix A (row-major, destroyed)
void JacobiEigenSym(int n, double *A, double *V, double *eig);
// A = U diag(s) V^T for a 3x3 matrix: s descending, U and V orthogonal (row-major)
void JacobiSvd3(const double A[9], double U[9], double s[3], double V[9]);

}  // namespace sdvl

#endif  // SDVL_HOMOGRAPHY_INIT_H_
