// bundle.h — extra/bundle.h and Map::BundleAdjustment (map.cc:844-869) on the host: the walk over the keyframe graph that picks the
// window, its flattening into the arrays sdvl_bundle_adjust takes (include/sdvl_hip.h), and the write-back.  g2o's part — both optimize()
// calls and the outlier test between them — runs on the device, one workgroup per window, any number of windows in one call.
#ifndef SDVL_BUNDLE_H_
#define SDVL_BUNDLE_H_

#include <memory>
#include <vector>

#include "frontend.h"

namespace sdvl {

// what Bundle::Local (bundle.cc:65-190) builds before initializeOptimization(), as flat arrays
struct BundleProblem {
  std::vector<std::shared_ptr<Frame>> kfs;      // vertices: the free local keyframes, then local keyframe 0 (:123) and fixed_kfs (:94-106)
  int n_free = 0;
  std::vector<std::shared_ptr<Point>> points;   // lpoints, :72-87
  // projections, :159-189, point and keyframe by index into the two lists above; depth: what the observation's frame measured there
  // (Feature::GetDepth), filled in for a window collected with depth edges, 0 otherwise
  std::vector<sdvl_bundle_edge_depth> edges;
  int n_depth_edges = 0;     // edges that carry a depth
  int n_depth_level1 = 0;    // of them, those the outlier test moved to level 1 (Bundle::Solve)
  bool Empty() const { return kfs.empty(); }
};

// Depth edges (SDVL::SetDepthBundle): features of new keyframes handed to sdvl_depth_lookup, their lookups by status (sdvl_depth_seed's codes, [0] = OK), observations
// that got a depth stored (the looked-up ones and the seeded corners), and for the last window and all windows so far: edges, edges with
// a depth, depth edges that ended on level 1
struct DepthBundleStats {
  long features = 0, lookups[5] = {0, 0, 0, 0, 0}, stored = 0;
  long last_edges = 0, last_depth_edges = 0, last_depth_level1 = 0;
  long total_edges = 0, total_depth_edges = 0, total_depth_level1 = 0;
};

// runs, skipped windows (more free poses than the device takes), and the last window's sizes and result (sdvlh_batch_bundle_stats)
struct BundleStats {
  long runs = 0, skipped = 0;
  int n_free = 0, n_fixed = 0, n_points = 0, n_edges = 0;
  sdvl_bundle_result last = {};
};

class Bundle {
 public:
  // bundle.cc:65-190: the points of the local keyframes `kfs`, the other keyframes that see them, one edge per observation.  false: no
  // point (:91-92).  Deviation: a point seen twice from one keyframe contributes its first observation there (sdvl_bundle_adjust takes one
  // edge per pair; g2o would add both).
  // with_depth: the edges take the depth their observation carries (an edge without one stays a monocular edge)
  static bool Collect(const std::vector<std::shared_ptr<Frame>> &kfs, BundleProblem *out, bool with_depth = false);
  // both optimize() calls of every window in ONE sdvl_bundle_adjust call (bundle.cc:192-209).  results[j] and, for a window that ended
  // SDVL_BUNDLE_OK, Frame::SetPose for the poses that were optimised and Point::SetPosition for its points (:211-223); moved[j] = the
  // keyframes whose pose changed.
  // bf > 0: sdvl_bundle_adjust_depth with the windows' depths (a window collected without them has none: the monocular kernel runs it);
  // bf == 0: sdvl_bundle_adjust, the depths are not looked at.  Still one call.
  static void Solve(Device *dev, const Camera &camera, const std::vector<BundleProblem *> &problems, std::vector<sdvl_bundle_result> *results,
                    std::vector<std::vector<Frame *>> *moved, double bf = 0.0);

 private:
  static int NextId();  // Bundle::counter_, bundle.cc:39-49
};

}  // namespace sdvl

#endif  // SDVL_BUNDLE_H_
