// bundle.cc — Bundle::Local (extra/bundle.cc:65-224) around the device solver; see bundle.h.
#include "bundle.h"

#include <atomic>
#include <cstring>
#include <unordered_map>

namespace sdvl {

using std::shared_ptr;
using std::vector;

int Bundle::NextId() {
  static std::atomic<int> counter{0};
  return counter++;
}

bool Bundle::Collect(const vector<shared_ptr<Frame>> &kfs, BundleProblem *out, bool with_depth) {
  const int id = NextId();
  out->kfs.clear();
  out->points.clear();
  out->edges.clear();
  out->n_free = 0;
  out->n_depth_edges = out->n_depth_level1 = 0;
  // :72-87: all points involved.  (GetFeatures turns a tracked keyframe's flat records into Feature objects and links them to their points.)
  for (const shared_ptr<Frame> &kf : kfs) {
    kf->SetLastBA(id);
    for (const shared_ptr<Feature> &ft : kf->GetFeatures()) {
      const shared_ptr<Point> point = ft ? ft->GetPoint() : nullptr;
      if (!point || point->ToDelete()) continue;
      if (point->GetLastBA() != id) {
        point->SetLastBA(id);
        out->points.push_back(point);
      }
    }
  }
  if (out->points.empty()) return false;
  // :94-106: the keyframes that see these points, fixed
  vector<shared_ptr<Frame>> fixed_kfs;
  for (const shared_ptr<Point> &pt : out->points)
    for (const shared_ptr<Feature> &ft : pt->GetFeatures()) {
      const shared_ptr<Frame> frame = ft->GetFrame();
      if (frame && !frame->ToDelete() && frame->GetLastBA() != id) {
        frame->SetLastBA(id);
        fixed_kfs.push_back(frame);
      }
    }
  // :118-139: vertices; the device wants the free ones first, so local keyframe 0 (setFixed(id == 0)) moves behind them
  std::unordered_map<const Frame *, int32_t> index;
  for (const shared_ptr<Frame> &kf : kfs)
    if (kf->GetID() != 0 && index.emplace(kf.get(), static_cast<int32_t>(out->kfs.size())).second) out->kfs.push_back(kf);
  out->n_free = static_cast<int>(out->kfs.size());
  for (const shared_ptr<Frame> &kf : kfs)
    if (kf->GetID() == 0 && index.emplace(kf.get(), static_cast<int32_t>(out->kfs.size())).second) out->kfs.push_back(kf);
  for (const shared_ptr<Frame> &kf : fixed_kfs)
    if (index.emplace(kf.get(), static_cast<int32_t>(out->kfs.size())).second) out->kfs.push_back(kf);
  // :151-189: one edge per observation of every point from a keyframe that is a vertex
  vector<int32_t> seen(out->kfs.size(), -1);  // last point that got an edge to this keyframe
  for (size_t q = 0; q < out->points.size(); q++)
    for (const shared_ptr<Feature> &ft : out->points[q]->GetFeatures()) {
      const shared_ptr<Frame> frame = ft->GetFrame();
      if (!frame || frame->ToDelete()) continue;
      const auto it = index.find(frame.get());
      if (it == index.end()) continue;  // :167-168
      if (seen[it->second] == static_cast<int32_t>(q)) continue;
      seen[it->second] = static_cast<int32_t>(q);
      sdvl_bundle_edge_depth e;
      e.point = static_cast<int32_t>(q);
      e.keyframe = it->second;
      e.u = ft->GetPosition()(0);
      e.v = ft->GetPosition()(1);
      e.depth = with_depth ? ft->GetDepth() : 0.0;
      if (e.depth > 0.0) out->n_depth_edges++;
      out->edges.push_back(e);
    }
  return true;
}

void Bundle::Solve(Device *dev, const Camera &camera, const vector<BundleProblem *> &problems, vector<sdvl_bundle_result> *results,
                   vector<vector<Frame *>> *moved, double bf) {
  const int J = static_cast<int>(problems.size());
  results->assign(J, sdvl_bundle_result{});
  moved->assign(J, vector<Frame *>());
  if (J == 0) return;
  vector<sdvl_bundle_problem> ranges(J);
  vector<double> poses, points;
  vector<int32_t> fixed;
  vector<sdvl_bundle_edge_depth> edges;
  for (int j = 0; j < J; j++) {
    const BundleProblem &p = *problems[j];
    sdvl_bundle_problem &r = ranges[j];
    r.kf_begin = static_cast<int32_t>(fixed.size());
    r.pt_begin = static_cast<int32_t>(points.size() / 3);
    r.edge_begin = static_cast<int32_t>(edges.size());
    for (size_t k = 0; k < p.kfs.size(); k++) {
      double pose[7];
      p.kfs[k]->GetPose().ToArray(pose);  // :121, :133
      poses.insert(poses.end(), pose, pose + 7);
      fixed.push_back(static_cast<int>(k) < p.n_free ? 0 : 1);
    }
    for (const shared_ptr<Point> &pt : p.points) {
      const Vector3d x = pt->GetPosition();  // :153
      points.push_back(x(0)); points.push_back(x(1)); points.push_back(x(2));
    }
    edges.insert(edges.end(), p.edges.begin(), p.edges.end());
    r.kf_end = static_cast<int32_t>(fixed.size());
    r.pt_end = static_cast<int32_t>(points.size() / 3);
    r.edge_end = static_cast<int32_t>(edges.size());
  }
  vector<int32_t> levels(edges.size() + 1), pose_stages(fixed.size() + 1), point_stages(points.size() / 3 + 1);
  const sdvl_camera cam = camera.abi();  // :180-183
  if (bf > 0.0) {
    dev->Check(sdvl_bundle_adjust_depth(dev->ctx(), J, ranges.data(), static_cast<int>(fixed.size()), poses.data(), fixed.data(),
                                        static_cast<int>(points.size() / 3), points.data(), static_cast<int>(edges.size()), edges.data(), &cam, bf,
                                        levels.data(), pose_stages.data(), point_stages.data(), results->data()),
               "sdvl_bundle_adjust_depth");
  } else {
    vector<sdvl_bundle_edge> mono(edges.size());
    for (size_t e = 0; e < edges.size(); e++) mono[e] = sdvl_bundle_edge{edges[e].point, edges[e].keyframe, edges[e].u, edges[e].v};
    dev->Check(sdvl_bundle_adjust(dev->ctx(), J, ranges.data(), static_cast<int>(fixed.size()), poses.data(), fixed.data(), static_cast<int>(points.size() / 3),
                                  points.data(), static_cast<int>(mono.size()), mono.data(), &cam, levels.data(), pose_stages.data(), point_stages.data(),
                                  results->data()),
               "sdvl_bundle_adjust");
  }
  for (int j = 0; j < J; j++) {
    if ((*results)[j].status != SDVL_BUNDLE_OK) continue;  // the estimates stay as they were
    BundleProblem &p = *problems[j];
    const sdvl_bundle_problem &r = ranges[j];
    p.n_depth_level1 = 0;
    for (int e = r.edge_begin; e < r.edge_end && bf > 0.0; e++) p.n_depth_level1 += edges[e].depth > 0.0 && levels[e] != 0 ? 1 : 0;
    // :211-216 — poses first: a candidate point's position hangs off its first keyframe's pose (Point::SetPosition)
    for (int k = 0; k < p.n_free; k++) {
      if (!pose_stages[r.kf_begin + k]) continue;  // a vertex without an active edge was not optimised
      const double *np = poses.data() + 7 * static_cast<size_t>(r.kf_begin + k);
      double old[7];
      p.kfs[k]->GetPose().ToArray(old);
      if (std::memcmp(old, np, sizeof(old)) == 0) continue;
      p.kfs[k]->SetPose(SE3::FromArray(np));
      (*moved)[j].push_back(p.kfs[k].get());
    }
    // :218-223 — every point, optimised or not: a candidate keeps its world position when its first keyframe has moved
    for (size_t q = 0; q < p.points.size(); q++) {
      const double *x = points.data() + 3 * (static_cast<size_t>(r.pt_begin) + q);
      p.points[q]->SetPosition(Vector3d(x[0], x[1], x[2]));
    }
  }
}

}  // namespace sdvl
