// standalone.cc — the part of the host layer the reference's own tree already has: Camera (camera.cc), Point (point.cc), Map and
// the plane-map stub (map.cc), SDVL (sdvl.cc).  The hot path's classes are in frontend.cc; the batch driver SDVL::HandleFrame steps
// through, SDVLBatch, is in the batch*.cc files.  Reference line numbers are cited at each function; device work goes through the C-ABI
// (include/sdvl_hip.h) only.
#include "batch_internal.h"
#include "homography_init.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <mutex>
#include <stdexcept>

namespace sdvl {

using std::shared_ptr;
using std::vector;

// -------------------------------------------------------------------------------------------------------- Camera
Camera::Camera() {
  const CameraParameters &p = Config::GetCameraParameters();
  width_ = p.width; height_ = p.height; fx_ = p.fx; fy_ = p.fy; u0_ = p.u0; v0_ = p.v0;
  SetDistortions(p.d1, p.d2, p.d3, p.d4, p.d5);
}
Camera::Camera(int width, int height, double fx, double fy, double u0, double v0)
    : width_(width), height_(height), fx_(fx), fy_(fy), u0_(u0), v0_(v0) {}

// camera.cc:39-67
void Camera::SetDistortions(double d0, double d1, double d2, double d3, double d4) {
  d_[0] = d0; d_[1] = d1; d_[2] = d2; d_[3] = d3; d_[4] = d4;
  has_distortion_ = !(d_[0] == 0.0);
}

// camera.cc:100-105.  (an addition) A colour image (Image::format) is converted first, then undistorted — cv::cvtColor (video_source.cc:63)
// and then UndistortImage, the order of main.cc:128-137: the result is the undistorted GRAY image.
void Camera::UndistortImage(const Image &in, Image *out) const {
  Device *dev = Device::Current();
  if (!dev) throw std::runtime_error("Camera::UndistortImage: no sdvl::Device bound to this thread");
  const int w = in.cols, h = in.rows;
  void *buf = nullptr;
  dev->Check(sdvl_device_malloc(dev->ctx(), static_cast<int64_t>(w) * h, &buf), "sdvl_device_malloc");
  sdvl_ctx *ctx = dev->ctx();
  std::shared_ptr<void> owner(buf, [ctx](void *p) { sdvl_device_free(ctx, p); });
  const void *src = in.dev_src ? in.dev_src : static_cast<const void *>(in.data);
  const sdvl_camera cam = abi();
  const sdvl_distortion dist = distortion();  // d0 == 0 -> plain copy, like in.clone()
  if (in.color()) {
    if (!HasDistortion()) {
      dev->Check(sdvl_convert_gray(ctx, 1, &src, in.step, in.dev_src ? 1 : 0, w, h, in.format, &buf, w), "sdvl_convert_gray");
    } else {
      void *gray = nullptr;
      dev->Check(sdvl_device_malloc(ctx, static_cast<int64_t>(w) * h, &gray), "sdvl_device_malloc");
      std::shared_ptr<void> keep(gray, [ctx](void *p) { sdvl_device_free(ctx, p); });  // (sdvl_device_free waits for the stream)
      dev->Check(sdvl_convert_gray(ctx, 1, &src, in.step, in.dev_src ? 1 : 0, w, h, in.format, &gray, w), "sdvl_convert_gray");
      const void *gsrc = gray;
      dev->Check(sdvl_undistort(ctx, 1, &gsrc, w, 1, w, h, &cam, &dist, &buf, w), "sdvl_undistort");
    }
  } else {
    dev->Check(sdvl_undistort(ctx, 1, &src, in.step, in.dev_src ? 1 : 0, w, h, &cam, &dist, &buf, w), "sdvl_undistort");
  }
  *out = Image::WrapDevice(buf, w, h, w, false);
  out->dev_owner = owner;
}

// camera.cc:69-79
void Camera::Project(const Vector3d &p3D, Vector2d *p2D) const {
  (*p2D)(0) = u0_ + fx_ * p3D(0) / p3D(2);
  (*p2D)(1) = v0_ + fy_ * p3D(1) / p3D(2);
}
void Camera::Unproject(const Vector2d &p2D, Vector3d *p3D) const {
  const double x = (p2D(0) - u0_) / fx_, y = (p2D(1) - v0_) / fy_, z = 1.0;
  const double n = std::sqrt(x * x + y * y + z * z);
  (*p3D)(0) = x / n; (*p3D)(1) = y / n; (*p3D)(2) = z / n;
}

static std::atomic<int> g_point_counter{0};

// point.cc:32-43
Point::Point() {
  Device *cur = Device::CurrentOrNull();
  id_ = cur ? (*cur->point_ids)++ : g_point_counter++;
  status_ = P_NOT_FOUND;
  last_frame_ = -1;
  n_failed_ = 0;
  n_successful_ = 0;
  delete_ = false;
  fixed_ = false;
  a_ = b_ = 10;
  rho_ = 1.0;
  sigma2_ = 1.0;
  z_range_ = 6.0;
}
void Point::ConsumeId() {
  if (Device *cur = Device::CurrentOrNull()) (*cur->point_ids)++;
  else g_point_counter++;
}
double Point::GetStd() { return std::sqrt(sigma2_); }

// point.cc:48-62
void Point::InitCandidate(const shared_ptr<Feature> &p, double depth) {
  feature_ = p;
  a_ = 10; b_ = 10;
  rho_ = 1.0 / depth;
  sigma2_ = 1.0;
  z_range_ = std::sqrt(sigma2_ * 36);
}
void Point::InitFixed(const shared_ptr<Feature> &f, double depth, double sigma2, const Vector3d &p3d) {
  InitCandidate(f, depth);
  sigma2_ = sigma2;
  fixed_ = true;
  p3d_ = p3d;
}

void Point::GetFilterState(sdvl_depth_state *st) const {
  st->rho = rho_; st->sigma2 = sigma2_; st->a = a_; st->b = b_; st->z_range = z_range_;
  st->cos_alpha = cos_alpha_; st->last_distance = last_distance_;
  st->position[0] = p3d_(0); st->position[1] = p3d_(1); st->position[2] = p3d_(2);
  st->fixed = fixed_ ? 1 : 0;
  st->n_failed = n_failed_;
  st->track_row = track_row_;
  st->pad_ = 0;
}

// what Map::UpdateCandidates' loop body (map.cc:454-497) left of the point, computed by depth_filter_kernel
void Point::ApplyFilterOut(const sdvl_depth_out &o) {
  const int what = o.outcome & 0xFF;
  if (what == SDVL_DEPTH_NOT_FOUND) {  // Unpromote
    n_failed_ = o.n_failed;
    b_ = o.b;
  } else if (what == SDVL_DEPTH_UPDATED || what == SDVL_DEPTH_CONVERGED) {  // Update (+ HasConverged)
    rho_ = o.rho; sigma2_ = o.sigma2; a_ = o.a; b_ = o.b;
    cos_alpha_ = o.cos_alpha; last_distance_ = o.last_distance;
    n_failed_ = 0;
    if (what == SDVL_DEPTH_CONVERGED && !fixed_) {
      p3d_ = Vector3d(o.position[0], o.position[1], o.position[2]);
      fixed_ = true;
    }
  } else if (what == SDVL_DEPTH_FIXED_STALE && !fixed_) {  // Update returned early, HasConverged fixed the old estimate
    p3d_ = Vector3d(o.position[0], o.position[1], o.position[2]);
    fixed_ = true;
  }
}

// point.cc:128-142
Vector3d Point::GetPosition() const {
  if (fixed_) return p3d_;
  Frame *fr = feature_->GetFrameRaw();
  const SE3 se3 = fr->GetWorldPose();
  const Vector3d &v = feature_->GetVector();
  const double s = 1.0 / rho_;
  return se3 * Vector3d(s * v(0), s * v(1), s * v(2));
}

// point.cc:144-162
void Point::SetPosition(const Vector3d &pos) {
  if (fixed_) {
    p3d_ = pos;
    return;
  }
  shared_ptr<Frame> frame = feature_->GetFrame();
  Vector2d p2d;
  frame->Project(pos, &p2d);
  Vector3d v3d = frame->GetCamera()->Unproject(p2d);
  feature_->SetVector(v3d);
  rho_ = 1.0 / frame->DistanceTo(pos);
}

// point.cc:105-118
bool Point::Promote() { n_successful_++; n_failed_ = 0; return true; }
bool Point::Unpromote() {
  n_failed_++;
  b_++;
  return n_failed_ > Config::MaxFailed();
}

// ------------------------------------------------------------------------------------------------------------ Map
// map.cc:170-188
bool Map::NeedKeyframe(const shared_ptr<Frame> &frame, int) {
  const int npoints = frame->GetNumPoints();
  const bool enough_its = (frame->GetID() - last_kf_->GetID()) >= Config::MinKeyframeIts();
  const bool lost_many = npoints < last_matches_ * Config::LostRatio();
  const bool lost_some = npoints < last_matches_ * 0.9;
  last_matches_ = std::max(last_matches_, npoints);
  if ((enough_its && lost_some) || lost_many) {
    last_matches_ = npoints;
    return true;
  }
  return false;
}

// map.cc:145-159
void Map::AddKeyframe(const shared_ptr<Frame> &frame, bool) {
  version_++;
  keyframes_.push_back(frame);
  last_kf_ = frame;
}

// map.cc:207-259 (points)
void Map::EmptyTrash() {
  if (!points_trash_.empty()) version_++;
  for (auto &p : points_trash_) {
    if (!p->ToDelete() && p->TrackRow() >= 0 && !p->DeviceTrashed()) tables_dirty_ = true;
    std::list<shared_ptr<Feature>> &features = p->GetFeatures();
    for (auto it = features.begin(); it != features.end(); it++) (*it)->SetPoint(nullptr);
    features.clear();
    p->SetDelete();
  }
  points_trash_.clear();
}

// map.cc:190-205,692-706 for the plane-map stub (see sdvl_host.h)
void PlaneMap::LimitKeyframes(const shared_ptr<Frame> &frame) {
  if (static_cast<int>(keyframes_.size()) < Config::MaxKeyframes()) return;
  const Vector3d pos = frame->GetWorldPosition();
  shared_ptr<Frame> kf;
  double maxdist = 0.0;
  for (auto it = keyframes_.begin(); it != keyframes_.end(); it++) {
    const Vector3d q = (*it)->GetWorldPosition();
    const double dist = vnorm({q(0) - pos(0), q(1) - pos(1), q(2) - pos(2)});
    if (dist > maxdist) {
      maxdist = dist;
      kf = *it;
    }
  }
  if (!kf || kf == frame) return;
  kf->SetDelete();
  culled_.push_back(kf);
}

void PlaneMap::EmptyTrash() {
  if (!culled_.empty()) version_++;
  for (const shared_ptr<Frame> &kf : culled_) {
    // the points this keyframe seeded (their first observation is one of its features) go with it
    vector<shared_ptr<Feature>> &features = kf->GetFeatures();
    for (auto it = features.begin(); it != features.end(); it++) {
      if (!*it) continue;
      shared_ptr<Point> p = (*it)->GetPoint();
      if (p && !p->ToDelete() && p->GetInitFeature() == *it) DeletePoint(p);
    }
    for (auto it = keyframes_.begin(); it != keyframes_.end(); it++)
      if (*it == kf) {
        keyframes_.erase(it);
        break;
      }
  }
  Map::EmptyTrash();  // (clears the doomed points' feature lists, the culled keyframe's features among them)
  for (const shared_ptr<Frame> &kf : culled_) kf->RemoveFeatures();
  culled_.clear();
}

void PlaneMap::InitCandidates(const shared_ptr<Frame> &kf) {
  kf->FilterCorners();
  SeedFromFiltered(kf);
}

void PlaneMap::SeedFromFiltered(const shared_ptr<Frame> &kf) {
  const SE3 world = kf->GetWorldPose();
  const M3 Rw = world.GetRotation();
  const Vector3d tw = world.GetTranslation();
  const int n_filtered = kf->NumFiltered();
  for (int k = 0; k < n_filtered; k++) {
    const Vector3i corner = kf->FilteredCorner(k);
    const int scale = (1 << corner(2));
    shared_ptr<Feature> feature = kf->NewFeature(Vector2d(corner(0) * scale, corner(1) * scale), corner(2));
    if (Config::UseORB()) feature->SetDescriptor(kf->FilteredDescriptor(k));  // filled by FilterCorners (frame.cc:145-161)
    const Vector3d &v = feature->GetVector();
    const V3 ray = mvec(Rw, {v(0), v(1), v(2)});
    const double denom = n_(0) * ray.x + n_(1) * ray.y + n_(2) * ray.z;
    if (!(std::fabs(denom) > 1e-9)) continue;
    const double s = (d_ - (n_(0) * tw(0) + n_(1) * tw(1) + n_(2) * tw(2))) / denom;
    if (!(s > 0.05)) continue;
    shared_ptr<Point> pt = kf->NewPoint();
    const double rho = 1.0 / s;
    pt->InitFixed(feature, s, (0.05 * rho) * (0.05 * rho), world * Vector3d(s * v(0), s * v(1), s * v(2)));
    version_++;
    feature->SetPoint(pt);
    kf->AddFeature(feature);
    pt->AddFeature(feature);
  }
}

// Depth cameras: SeedFromFiltered with the scale from a registered depth image.  z is the camera-frame depth (along the optical axis), the
// bearing v is a unit vector, so the point lies at s = z / v_z along it; on a fronto-parallel plane seen from the identity pose that is the
// plane's (d - n.t) / (n.ray) with the same operands.  The `fixed` branch of Map::InitCandidates (map.cc:269,385-389) is what this feeds.
void PlaneMap::SeedFromDepth(const shared_ptr<Frame> &kf, const double *z, const uint8_t *status) {
  const SE3 world = kf->GetWorldPose();
  const int n_filtered = kf->NumFiltered();
  depth_seeds_.erase(std::remove_if(depth_seeds_.begin(), depth_seeds_.end(), [](const DepthSeedRec &r) { return r.point.expired(); }),
                     depth_seeds_.end());
  depth_stats_.keyframes++;
  for (int k = 0; k < n_filtered; k++) {
    depth_stats_.by_status[status[k] <= SDVL_DEPTH_SEED_OUTSIDE ? status[k] : SDVL_DEPTH_SEED_HOLE]++;
    if (status[k] != SDVL_DEPTH_SEED_OK) continue;
    const Vector3i corner = kf->FilteredCorner(k);
    const int scale = (1 << corner(2));
    shared_ptr<Feature> feature = kf->NewFeature(Vector2d(corner(0) * scale, corner(1) * scale), corner(2));
    if (Config::UseORB()) feature->SetDescriptor(kf->FilteredDescriptor(k));
    const Vector3d &v = feature->GetVector();
    const double s = z[k] / v(2);
    if (!(s > 0.05)) continue;
    shared_ptr<Point> pt = kf->NewPoint();
    const double rho = 1.0 / s;
    pt->InitFixed(feature, s, (0.05 * rho) * (0.05 * rho), world * Vector3d(s * v(0), s * v(1), s * v(2)));
    version_++;
    feature->SetPoint(pt);
    kf->AddFeature(feature);
    pt->AddFeature(feature);
    depth_seeds_.push_back(DepthSeedRec{pt, kf->GetID(), corner(0), corner(1), corner(2)});
    depth_stats_.seeds++;
    if (store_depths_) {
      feature->SetDepth(z[k]);
      depth_bundle_stats_.stored++;
    }
  }
}

vector<PlaneMap::SeededPoint> PlaneMap::GetSeededPoints() const {
  vector<SeededPoint> out;
  for (const DepthSeedRec &r : depth_seeds_) {
    const shared_ptr<Point> p = r.point.lock();
    if (!p || p->ToDelete()) continue;
    const Vector3d pos = p->GetPosition();
    out.push_back(SeededPoint{pos(0), pos(1), pos(2), r.keyframe_id, r.u, r.v, r.level});
  }
  return out;
}

// ----------------------------------------------------------------------------------------------------------- SDVL
SDVL::SDVL(Camera *camera, Map *map, const SE3 &first_pose)
    : camera_(camera), map_(map), rng_(1), feature_align_(map, camera, Config::MaxMatches(), &rng_), first_pose_(first_pose) {}

static Device *OwnDeviceIfNone() {
  if (Device::CurrentOrNull()) return nullptr;
  const char *g = std::getenv("SDVL_GPU");
  return new Device(g ? std::atoi(g) : 0);  // binds itself to the thread
}

// sdvl.cc:36-50
SDVL::SDVL(Camera *camera)
    : own_device_(OwnDeviceIfNone()),
      own_map_(new MapperMap(Vector3d(0.0, 0.0, 1.0), Config::MapScale(), camera)),
      camera_(camera),
      map_(own_map_.get()),
      rng_(1),
      feature_align_(map_, camera, Config::MaxMatches(), &rng_),
      first_pose_(SE3()) {}

SDVL::~SDVL() {
  if (own_map_) own_map_->Stop();
  self_batch_.reset();  // its tracking tables go before the frames and the device do
  current_frame_.reset();
  last_frame_.reset();
  last_kf_.reset();
  pending_kf_.reset();
  own_map_.reset();     // frames go back to the device's pool before the device does
}

void SDVL::SetBootstrapPlane(const Vector3d &n, double d) {
  if (PlaneMap *pm = dynamic_cast<PlaneMap *>(map_)) pm->SetPlane(n, d);
}

// the Point counters and feature lists HandleFrame's batch keeps on the device reach the host objects the queries below read
void SDVL::SyncSelfBatch() {
  if (self_batch_) self_batch_->SyncHostState();
}

const StageTimes *SDVL::HandleFrameStageTimes() const { return self_batch_ ? &self_batch_->stage_times : nullptr; }

// sdvl.cc:283-291
void SDVL::GetCameraTrail(vector<std::pair<SE3, bool>> *positions) {
  std::unique_lock<std::mutex> lock(map_->GetMutex());
  positions->clear();
  for (auto it = map_->GetKeyframes().begin(); it != map_->GetKeyframes().end(); it++)
    positions->push_back(std::make_pair((*it)->GetWorldPose(), (*it)->IsSelected()));
}

// sdvl.cc:293-324: converged points twice, the others as the two ends of their depth interval
void SDVL::GetPoints(vector<Vector3d> *positions) {
  std::unique_lock<std::mutex> lock(map_->GetMutex());
  SyncSelfBatch();
  positions->clear();
  for (auto it = map_->GetKeyframes().begin(); it != map_->GetKeyframes().end(); it++) {
    for (auto feature = (*it)->GetFeatures().begin(); feature != (*it)->GetFeatures().end(); feature++) {
      shared_ptr<Point> p = (*feature)->GetPoint();
      if (!p || p->ToDelete()) continue;
      if (p->HasConverged()) {
        positions->push_back(p->GetPosition());
        positions->push_back(p->GetPosition());
      } else {
        const double zmin = 1.0 / (p->GetInverseDepth() + 2.0 * p->GetStd());
        const double zmax = 1.0 / (std::max(p->GetInverseDepth() - 2.0 * p->GetStd(), 0.00000001));
        const Vector3d &v = p->GetInitFeature()->GetVector();
        const SE3 pose = p->GetInitFeature()->GetFrame()->GetWorldPose();
        positions->push_back(pose * Vector3d(v(0) * zmin, v(1) * zmin, v(2) * zmin));
        positions->push_back(pose * Vector3d(v(0) * zmax, v(1) * zmax, v(2) * zmax));
      }
    }
  }
}

// sdvl.cc:326-349: (x, y, Point status) of the last frame's features, then its outliers as status P_OUTLIER
void SDVL::GetLastFeatures(vector<Vector3i> *positions) {
  std::unique_lock<std::mutex> lock(map_->GetMutex());
  SyncSelfBatch();
  positions->clear();
  if (!last_frame_) return;
  vector<shared_ptr<Feature>> &features = last_frame_->GetFeatures();
  for (auto feature = features.begin(); feature != features.end(); feature++) {
    shared_ptr<Point> point = (*feature)->GetPoint();
    if (!point || point->ToDelete()) continue;
    const Vector2d &pos = (*feature)->GetPosition();
    positions->push_back(Vector3i(static_cast<int>(pos(0)), static_cast<int>(pos(1)), static_cast<int>(point->GetStatus())));
  }
  vector<Vector2d> &outliers = last_frame_->GetOutliers();
  for (auto it = outliers.begin(); it != outliers.end(); it++)
    positions->push_back(Vector3i(static_cast<int>((*it)(0)), static_cast<int>((*it)(1)), static_cast<int>(Point::P_OUTLIER)));
}

SE3 SDVL::GetPose() const {
  if (last_frame_) return last_frame_->GetWorldPose();
  return SE3();
}

// sdvl.cc:240-264
void SDVL::CalcTrackingQuality(int matches, int attempts) {
  const double ratio = (attempts == 0) ? 0.0 : static_cast<double>(matches) / static_cast<double>(attempts);
  if (ratio > 0.2) {
    tracking_quality_ = TRACKING_GOOD;
    lost_frames_ = 0;
    return;
  }
  if (matches < Config::MinMatches()) {
    tracking_quality_ = TRACKING_BAD;
    lost_frames_++;
    return;
  }
  lost_frames_ = 0;
  tracking_quality_ = TRACKING_INSUFFICIENT;
}

// sdvl.cc:278-281
void SDVL::SetMotionModel() { current_frame_->SetPose(SE3::Exp(vel_) * last_frame_->GetPose()); }

// sdvl.cc:266-276
void SDVL::GetMotionModel() {
  const SE3 mov = current_frame_->GetPose() * last_frame_->GetPose().Inverse();
  const Vector6d vel = SE3::Log(mov);
  for (int c = 0; c < 6; c++) vel_[c] = 0.9 * (0.5 * vel[c] + 0.5 * vel_[c]);
}

// sdvl.h:85
void SDVL::ResetMotionModel() {
  for (int k = 0; k < 6; k++) vel_[k] = 0.0;
}

// bootstrap replacement (SaveFirstFrame/SaveSecondFrame are out of scope): first frame = keyframe at first_pose
void SDVL::SaveFirstFrame(FrameStats &st) {
  current_frame_->SetPose(first_pose_);
  current_frame_->SetKeyframe();
  map_->AddKeyframe(current_frame_, false);  // like SaveFirstFrame / SaveSecondFrame (sdvl.cc:144,165): not queued
  pending_kf_ = current_frame_;              // seeded from the scene plane in the mapping stage
  last_frame_ = current_frame_;
  last_kf_ = current_frame_;
  state_ = STATE_RUNNING;
  track_.valid = false;
  st.state = 0;
  st.keyframe = 1;
}

// SaveFirstFrame for a tracker that seeds from depth: whether the frame becomes the first keyframe is known once its filtered corners have
// been looked up in the depth image (SDVLBatch::FinishKeyframes)
void SDVL::PrepareFirstFrame() {
  current_frame_->SetPose(first_pose_);
  pending_kf_ = current_frame_;
  first_frame_waiting_ = true;
}

void SDVL::CommitFirstFrame(FrameStats &st) {
  first_frame_waiting_ = false;
  current_frame_->SetKeyframe();
  map_->AddKeyframe(current_frame_, false);
  last_frame_ = current_frame_;
  last_kf_ = current_frame_;
  state_ = STATE_RUNNING;
  track_.valid = false;
  st.state = 0;
  st.keyframe = 1;
}

void SDVL::SetDepthSeeding(bool on, const sdvl_depth_seed_params &rule) {
  if (on && two_frame_init_) throw std::runtime_error("SDVL::SetDepthSeeding: the tracker takes the two-frame initialisation; the two answer the same question");
  if (on && !dynamic_cast<PlaneMap *>(map_)) throw std::runtime_error("SDVL::SetDepthSeeding needs a PlaneMap or the reference's mapper (MapperMap)");
  if (on && (rule.edge_ratio < 0.0 || rule.min_valid < 0 || rule.min_valid > 9))
    throw std::invalid_argument("SDVL::SetDepthSeeding: edge_ratio is negative or min_valid lies outside 1 .. 9");
  if (on && stereo_seeding_) throw std::runtime_error("SDVL::SetDepthSeeding: the tracker seeds from a stereo pair (SetStereoSeeding); a frame brings one second image");
  if (MapperMap *m = dynamic_cast<MapperMap *>(map_))
    if (!on && m->StereoMapping()) throw std::runtime_error("SDVL::SetDepthSeeding: stereo mapping is on (SetStereoMapping) and needs the stereo seeding this turns off");
  depth_seeding_ = on;
  depth_rule_ = rule;
  if (!on) {
    stereo_seeding_ = false;
    camera_->SetRectifiedPair(nullptr);  // the raw pairs go with the switch that reads them
  }
}

void SDVL::SetStereoSeeding(bool on, double baseline, const sdvl_stereo_params &rule) {
  if (on && two_frame_init_) throw std::runtime_error("SDVL::SetStereoSeeding: the tracker takes the two-frame initialisation; the two answer the same question");
  if (on && !dynamic_cast<PlaneMap *>(map_)) throw std::runtime_error("SDVL::SetStereoSeeding needs a PlaneMap or the reference's mapper (MapperMap)");
  if (on && depth_seeding_ && !stereo_seeding_)
    throw std::runtime_error("SDVL::SetStereoSeeding: the tracker seeds from a depth image (SetDepthSeeding); a frame brings one second image");
  if (MapperMap *m = dynamic_cast<MapperMap *>(map_))
    if (!on && m->StereoMapping()) throw std::runtime_error("SDVL::SetStereoSeeding: stereo mapping is on (SetStereoMapping) and needs stereo seeding");
  if (MapperMap *m = dynamic_cast<MapperMap *>(map_))
    if (on && (m->DepthMapping() || m->DepthBundleOn()))
      throw std::runtime_error("SDVL::SetStereoSeeding: depth mapping and depth edges look depths up at found pixels, which a matcher at the corners does not give");
  if (on && camera_->HasDistortion())
    throw std::runtime_error("SDVL::SetStereoSeeding: the camera has a lens; rectified pairs only (for a calibrated rig build the camera from "
                             "RectifiedPair::camera() and call SetStereoRectification)");
  if (on && !(baseline > 0.0 && std::isfinite(baseline))) throw std::invalid_argument("SDVL::SetStereoSeeding: the baseline is not a positive finite number");
  if (on && (rule.max_disparity < 0 || rule.max_disparity > SDVL_STEREO_MAX_DISPARITY || rule.uniqueness < 0 || rule.uniqueness > 100 || rule.max_sad < 0 ||
             rule.max_sad > 255 || !(rule.min_depth >= 0.0 && std::isfinite(rule.min_depth)) || !(rule.max_depth >= 0.0 && std::isfinite(rule.max_depth))))
    throw std::invalid_argument("SDVL::SetStereoSeeding: max_disparity above 511, uniqueness outside 1 .. 100, max_sad outside 1 .. 255 or a negative depth");
  depth_seeding_ = on;
  stereo_seeding_ = on;
  stereo_rule_ = rule;
  stereo_rule_.baseline = baseline;
  stereo_rule_.dist = nullptr;
  if (!on) camera_->SetRectifiedPair(nullptr);  // the raw pairs go with the switch that reads them
}

void SDVL::SetStereoRectification(const RectifiedPair &pair, bool on) {
  if (!on) {
    camera_->SetRectifiedPair(nullptr);
    return;
  }
  if (!stereo_seeding_) throw std::runtime_error("SDVL::SetStereoRectification needs stereo seeding (SetStereoSeeding): the right image is its");
  if (camera_->HasDistortion())
    throw std::runtime_error("SDVL::SetStereoRectification: the camera has a lens of its own; the tracker's camera is the pair's rectified camera, the lenses are the pair's");
  const sdvl_camera have = camera_->abi(), &want = pair.camera();
  if (have.fx != want.fx || have.fy != want.fy || have.u0 != want.u0 || have.v0 != want.v0 || have.width != pair.width || have.height != pair.height)
    throw std::runtime_error("SDVL::SetStereoRectification: the camera's intrinsics or size differ from the pair's; build the camera from RectifiedPair::camera()");
  if (!(std::fabs(stereo_rule_.baseline - pair.baseline) <= 1e-12 * pair.baseline))
    throw std::runtime_error("SDVL::SetStereoRectification: the baseline of SetStereoSeeding differs from the pair's");
  if (MapperMap *m = dynamic_cast<MapperMap *>(map_))
    if (m->IsThreaded()) throw std::runtime_error("SDVL::SetStereoRectification: the mapper thread is started; raw pairs are rectified in sequential mode only");
  camera_->SetRectifiedPair(&pair);
}

void SDVL::SetDepthMapping(bool on, double noise_abs, double noise_quad) {
  MapperMap *m = AsMapperMap(map_);
  if (on && !m) throw std::runtime_error("SDVL::SetDepthMapping needs the reference's mapper (MapperMap)");
  if (on && stereo_seeding_) throw std::runtime_error("SDVL::SetDepthMapping: the tracker seeds from a stereo pair (SetStereoSeeding), which gives no depth at a found pixel");
  if (on && !depth_seeding_) throw std::runtime_error("SDVL::SetDepthMapping needs depth seeding (SetDepthSeeding): the bootstrap keyframe is seeded from depth too");
  if (m) m->SetDepthMapping(on, noise_abs, noise_quad);
}

void SDVL::SetStereoMapping(bool on, double disparity_sigma) {
  MapperMap *m = AsMapperMap(map_);
  if (on && !m) throw std::runtime_error("SDVL::SetStereoMapping needs the reference's mapper (MapperMap)");
  if (on && !stereo_seeding_) throw std::runtime_error("SDVL::SetStereoMapping needs stereo seeding (SetStereoSeeding): the baseline, the rule and the bootstrap keyframe are its");
  if (m) m->SetStereoMapping(on, disparity_sigma, camera_->abi().fx * stereo_rule_.baseline);
}

void SDVL::SetDepthBundle(bool on, double bf) {
  MapperMap *m = dynamic_cast<MapperMap *>(map_);
  if (on && !m) throw std::runtime_error("SDVL::SetDepthBundle needs the reference's mapper (MapperMap)");
  if (on && stereo_seeding_) throw std::runtime_error("SDVL::SetDepthBundle: the tracker seeds from a stereo pair (SetStereoSeeding), which gives no depth at a found pixel");
  if (on && !depth_seeding_) throw std::runtime_error("SDVL::SetDepthBundle needs depth seeding (SetDepthSeeding): without it no observation carries a depth");
  if (m) m->SetDepthBundle(on, bf);
}

void SDVL::SetBundleAdjustment(bool on) {
  MapperMap *m = AsMapperMap(map_);
  if (!m) throw std::runtime_error("SDVL::SetBundleAdjustment needs the reference's mapper (MapperMap)");
  m->SetBundleAdjustment(on);
}

void SDVL::SetTwoFrameInit(bool on) {
  if (on && !AsMapperMap(map_)) throw std::runtime_error("SDVL::SetTwoFrameInit needs the reference's mapper (MapperMap)");
  if (on && depth_seeding_) throw std::runtime_error("SDVL::SetTwoFrameInit: the tracker seeds from depth (SetDepthSeeding); the two answer the same question");
  two_frame_init_ = on;
  if (on && !h_init_) h_init_.reset(new HomographyInit(map_, Config::MinAvgShift()));
}

// sdvl.cc:132-148
bool SDVL::InitFirstFrame(FrameStats &st) {
  st.state = 0;
  current_frame_->CreateCorners(Config::MaxFastLevels(), 2 * Config::NumFeatures());
  current_frame_->SetPose(SE3());
  last_frame_ = current_frame_;  // sdvl.cc:63-64
  last_kf_ = current_frame_;
  track_.valid = false;
  if (!h_init_->InitFirstFrame(current_frame_)) return false;
  current_frame_->SetKeyframe();
  map_->AddKeyframe(current_frame_, false);
  state_ = STATE_SECOND_FRAME;
  st.keyframe = 1;
  return true;
}

// sdvl.cc:154-176 behind HomographyInit::InitSecondFrame, and :66-71
void SDVL::SecondFrameDone(bool initialised, FrameStats &st) {
  st.state = 1;
  track_.valid = false;
  if (!initialised) {
    if (h_init_->HasError()) {  // :155-158, :66-69: the reference is lost for good here; this tracker starts over (stated deviation)
      std::cerr << "[ERROR] Homography couldn't be performed" << std::endl;
      h_init_->Reset();
      state_ = STATE_FIRST_FRAME;
      init_failed_ = true;
      st.state = 0;
      return;
    }
    last_frame_ = current_frame_;  // :160 returns true: :70-71 run
    last_kf_ = current_frame_;
    return;
  }
  current_frame_->SetKeyframe();  // :164-165
  map_->AddKeyframe(current_frame_, false);
  // (Map::TransformInitialMap, :168-170, is not built: the world frame stays the first camera's)
  // :172, map_.BundleAdjustment() without UpdateMap's size test: the second keyframe has no connections yet (CheckConnections runs in its
  // mapper update), so the window is that keyframe alone and Map::BundleAdjustment returns at map.cc:860 with the keyframe still waiting
  if (MapperMap *m = AsMapperMap(map_)) m->BundleAdjustment(0);
  h_init_->Reset();
  state_ = STATE_RUNNING;
  last_frame_ = current_frame_;
  last_kf_ = current_frame_;
  st.state = 2;
  st.keyframe = 1;
}

// sdvl.cc:97-100: CalcTrackingQuality, then NeedKeyframe.  0 = tracking lost, 1 = ordinary frame, 2 = new keyframe
int SDVL::TrackingDecision() {
  CalcTrackingQuality(matches_, attempts_);
  if (tracking_quality_ == TRACKING_BAD) return 0;
  return (tracking_quality_ == TRACKING_GOOD && map_->NeedKeyframe(current_frame_, matches_)) ? 2 : 1;
}

// sdvl.cc:77-80: relocalisation starts (lost_frames_ >= 3)
void SDVL::StartRelocalizing() {
  map_->SetRelocalizing(true);
  ResetMotionModel();
}

// sdvl.cc:84-85: relocalised onto keyframe kf
void SDVL::Relocalized(const shared_ptr<Frame> &kf, FrameStats &st) {
  map_->SetRelocalizing(false);
  last_kf_ = kf;
  last_frame_ = kf;
  track_.valid = false;  // the table follows last_frame_
  st.relocalized = 1;
}

// sdvl.cc:101-106: the points learn of their observations in the new keyframe
void SDVL::LinkFeatures() {
  vector<shared_ptr<Feature>> &features = current_frame_->GetFeatures();
  for (auto it = features.begin(); it != features.end(); it++)
    if (Point *p = (*it)->GetPointRaw()) p->AddFeature(*it);
}

// sdvl.cc:108-114: the frame becomes a keyframe
void SDVL::SaveKeyframe(FrameStats &st) {
  current_frame_->SetKeyframe();
  map_->AddKeyframe(current_frame_);
  last_kf_ = current_frame_;
  map_->LimitKeyframes(current_frame_);
  if (!AsMapperMap(map_)) pending_kf_ = current_frame_;  // plane map stub: seed every keyframe
  st.keyframe = 1;
}

void SDVL::SetNextImage(const Image &next) {
  next_image_.assign(1, next);
}

bool SDVL::HandleFrame(const Image &img) { return HandleFrame(img, DepthImage()); }

bool SDVL::HandleFrame(const Image &img, const DepthImage &depth) {
  std::unique_lock<std::mutex> lock(map_->GetMutex());  // the mapper thread of threaded mode stays out meanwhile
  FrameStats st;
  Device *dev = Device::Current();
  if (!self_batch_ || self_batch_->dev_ != dev) {  // first call, or the caller moved to another Device (= stream)
    if (self_batch_) self_batch_->SyncHostState();
    self_batch_.reset(new SDVLBatch(dev, {this}, 1));
    track_.valid = false;
  }
  if (!next_image_.empty()) {
    self_batch_->SetNextImages(next_image_);
    next_image_.clear();
  }
  try {
    self_batch_->HandleFrames({img}, depth.empty() ? std::vector<DepthImage>() : std::vector<DepthImage>{depth}, &st);
  } catch (...) {
    // a step that failed half way leaves the set's tables and its own bookkeeping in an unknown state: the next call starts with a
    // fresh batch and rebuilds the table from the host objects
    self_batch_.reset();
    track_.valid = false;
    throw;
  }
  return !init_failed_;  // sdvl.cc:66-69
}

void SDVL::Mapping() {
  std::unique_lock<std::mutex> lock(map_->GetMutex());
  if (pending_kf_) {
    PlaneMap *pm = dynamic_cast<PlaneMap *>(map_);
    if (pm) {
      pending_kf_->FilterCorners();
      pm->SeedFromFiltered(pending_kf_);
    } else {
      map_->InitCandidates(pending_kf_);
    }
    pending_kf_ = nullptr;
  }
  if (MapperMap *m = AsMapperMap(map_)) m->UpdateMap();  // main.cc:148-149
}

}  // namespace sdvl
