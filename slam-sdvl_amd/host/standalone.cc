// standalone.cc — the part of the host layer the reference's own tree already has: Camera (camera.cc), Point (point.cc), Map and
// the plane-map stub (map.cc), SDVL (sdvl.cc) and, on top, the batch driver SDVLBatch (B trackers per submission, device-resident
// tracking tables).  The hot path's classes are in frontend.cc.  SDVLBatch's sections, in this order: worker pool and switches; the
// tracking tables (SyncStats, BuildTable, AppendSeeds, UploadTables); the pieces every form of a step shares (Step, BeginFrame,
// DetectOnSideStream, CollectKeyframes); relocalisation inside the tabled step; the step on the tables (HandleFramesTracked) and
// HandleFrames; the host-driven step (HandleFramesGeneric); what follows the decisions (EpilogueAndMapper, FinishKeyframes, RunMappers).
// Reference line numbers are cited at each function; device work goes through the C-ABI (include/sdvl_hip.h) only.
#include "sdvl_host.h"
#include "homography_init.h"
#include "host_internal.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <new>
#include <stdexcept>
#include <chrono>
#include <thread>

#include <sys/mman.h>

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

void SDVL::SetBundleAdjustment(bool on) {
  MapperMap *m = dynamic_cast<MapperMap *>(map_);
  if (!m) throw std::runtime_error("SDVL::SetBundleAdjustment needs the reference's mapper (MapperMap)");
  m->SetBundleAdjustment(on);
}

void SDVL::SetTwoFrameInit(bool on) {
  if (on && !dynamic_cast<MapperMap *>(map_)) throw std::runtime_error("SDVL::SetTwoFrameInit needs the reference's mapper (MapperMap)");
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
  if (MapperMap *m = dynamic_cast<MapperMap *>(map_)) m->BundleAdjustment(0);
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
  if (!dynamic_cast<MapperMap *>(map_)) pending_kf_ = current_frame_;  // plane map stub: seed every keyframe
  st.keyframe = 1;
}

void SDVL::SetNextImage(const Image &next) {
  next_image_.assign(1, next);
}

bool SDVL::HandleFrame(const Image &img) {
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
    self_batch_->HandleFrames({img}, &st);
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
  if (MapperMap *m = dynamic_cast<MapperMap *>(map_)) m->UpdateMap();  // main.cc:148-149
}

// ------------------------------------------------------------------------------------------------------ SDVLBatch
namespace {
// persistent worker pool for the per-sequence host stages
class Pool {
 public:
  explicit Pool(int n) : stop_(false), gen_(0), pending_(0) {
    for (int i = 0; i < n; i++) workers_.emplace_back([this] { Run(); });
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : workers_) t.join();
  }
  void For(int n, const std::function<void(int)> &fn) {
    if (n <= 0) return;
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn;
      n_ = n;
      dev_ = Device::CurrentOrNull();
      next_.store(0);
      pending_ = static_cast<int>(workers_.size());
      gen_++;
    }
    cv_.notify_all();
    Drain();
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this] { return pending_ == 0; });
    if (err_) {
      std::exception_ptr e = err_;
      err_ = nullptr;
      std::rethrow_exception(e);
    }
  }

 private:
  void Drain() {
    for (;;) {
      const int i = next_.fetch_add(1);
      if (i >= n_) break;
      try {
        (*fn_)(i);
      } catch (...) {
        std::lock_guard<std::mutex> lk(m_);
        if (!err_) err_ = std::current_exception();
      }
    }
  }
  void Run() {
    unsigned seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
        Device::SetCurrent(dev_);  // the helpers work for the caller's device (Point ids, scratch) and on its GPU
      }
      Drain();
      {
        std::lock_guard<std::mutex> lk(m_);
        if (--pending_ == 0) done_.notify_all();
      }
    }
  }
  std::vector<std::thread> workers_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  bool stop_;
  unsigned gen_;
  int pending_;
  const std::function<void(int)> *fn_ = nullptr;
  Device *dev_ = nullptr;
  int n_ = 0;
  std::atomic<int> next_{0};
  std::exception_ptr err_;
};
}  // namespace

static Pool *g_pool_of(void *&slot, int threads) {
  if (!slot && threads > 1) slot = new Pool(threads - 1);
  return static_cast<Pool *>(slot);
}

SDVLBatch::SDVLBatch(Device *dev, const vector<SDVL *> &trackers, int host_threads) : dev_(dev), trk_(trackers), threads_(host_threads) {
  for (size_t i = 0; i < trk_.size(); i++) trk_[i]->track_.slot = static_cast<int>(i);
  const auto pfor = [this](int n, const std::function<void(int)> &fn) { ParallelFor(n, fn); };
  pfor_ = pfor;
  pfor_ref_ = pfor;
  // A lone camera (a batch of up to four) waits for chains of 0.2 ms: its context polls without sleeping for the first 500 us of a wait (a
  // sleeping poll wakes ~15 us late).  Larger batches keep the sleeping polls: their host threads need the CPU, and a farm waits ~9 ms.
  const int spin_us = trk_.size() <= 4 ? 500 : 0;
  if (dev_ && dev_->ctx()) (void)sdvl_ctx_set_wait_spin(dev_->ctx(), spin_us);
}
SDVLBatch::~SDVLBatch() {
  if (track_) {
    Device::SetCurrent(dev_);
    sdvl_track_destroy(dev_->ctx(), track_);
  }
  if (reloc_store_) {
    Device::SetCurrent(dev_);
    (void)sdvl_align_store_destroy(dev_->ctx(), reloc_store_);
  }
}

static thread_local void *g_pool_slot = nullptr;
static thread_local int g_pool_threads = 0;

void SDVLBatch::ParallelFor(int n, const std::function<void(int)> &fn) {
  if (threads_ <= 1 || n <= 1) {
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  if (g_pool_slot && g_pool_threads != threads_) {
    delete static_cast<Pool *>(g_pool_slot);
    g_pool_slot = nullptr;
  }
  g_pool_threads = threads_;
  g_pool_of(g_pool_slot, threads_)->For(n, fn);
}

void SDVLBatch::SetNextImages(const vector<Image> &next) { next_imgs_ = next; }

// process-wide switches: worker threads read them while a setter may write; -1 = the environment decides (read once)
static std::atomic<int> g_device_pose{-1};
void SDVLBatch::SetDevicePose(bool on) { g_device_pose = on ? 1 : 0; }
bool SDVLBatch::DevicePose() {
  static const int env = [] {
    const char *e = std::getenv("SDVL_POSE_HOST");
    return (e && e[0] == '1') ? 0 : 1;
  }();
  const int v = g_device_pose;
  return (v < 0 ? env : v) != 0;
}

static std::atomic<int> g_track_tables{-1};
void SDVLBatch::SetTrackTables(bool on) { g_track_tables = on ? 1 : 0; }
bool SDVLBatch::TrackTables() {
  static const int env = std::getenv("SDVL_NO_TRACK_TABLES") ? 0 : 1;
  const int v = g_track_tables;
  return (v < 0 ? env : v) != 0;
}

// The counters the device advanced (Promote / Unpromote / SetLastFrame / status) reach the Point objects.
void SDVLBatch::SyncStats(SDVL &t) {
  SDVL::TrackState &ts = t.track_;
  if (!ts.stats_dirty || !ts.points) return;
  const size_t n = std::min(ts.stats.size(), ts.points->size());
  for (size_t p = 0; p < n; p++) {
    const sdvl_track_point_stat &s = ts.stats[p];
    (*ts.points)[p]->SetTrackCounters(s.score, s.n_failed, s.last_frame, static_cast<Point::PointStatus>(s.status & 0xFF));
  }
  ts.stats_dirty = false;
}

void SDVLBatch::SyncHostState() {
  for (SDVL *t : trk_) {
    SyncStats(*t);
    if (t->last_frame_ && t->last_frame_->HasFlatFeatures()) t->last_frame_->GetFeatures();
  }
}

// a point, first observed as feature `init` of keyframe `ref`, as a table row (include/sdvl_hip.h: sdvl_track_point)
static inline void PointRow(Point *pt, Feature *init, Frame *ref, sdvl_track_point *row) {
  sdvl_track_point &tp = *row;
  const Vector3d P = pt->GetPosition();
  tp.position[0] = P(0); tp.position[1] = P(1); tp.position[2] = P(2);
  tp.px[0] = init->GetPosition()(0); tp.px[1] = init->GetPosition()(1);
  tp.bearing[0] = init->GetVector()(0); tp.bearing[1] = init->GetVector()(1); tp.bearing[2] = init->GetVector()(2);
  tp.idepth = pt->GetInverseDepth();
  tp.idepth_std = pt->GetStd();
  tp.ref = ref->device();
  tp.level = init->GetLevel();
  tp.fixed = pt->IsFixed() ? 1 : 0;
  tp.score = pt->Score();
  tp.n_failed = pt->GetFailed();
  tp.last_frame = pt->GetLastFrame();
  tp.status = static_cast<int32_t>(pt->GetStatus());
  if (init->HasDescriptor()) std::memcpy(tp.desc, init->DescriptorData().data(), 32);
  else std::memset(tp.desc, 0, 32);
}

// last_frame's features and the points behind them as table rows (include/sdvl_hip.h: sdvl_track_point / _feature).
// false: something the tables cannot express (a point without a first observation or whose keyframe is gone) — the step
// then runs on the host path.
bool SDVLBatch::BuildTable(SDVL &t) {
  SyncStats(t);
  vector<sdvl_track_point> *points = &t.track_.up_points;
  vector<sdvl_track_feature> *feats = &t.track_.up_feats;
  points->clear();
  feats->clear();
  t.track_.up_register.clear();
  vector<shared_ptr<Feature>> &features = t.last_frame_->GetFeatures();
  // the alignment stage takes at most SDVL_MAX_ALIGN_FEATURES features per job: a frame with more (a keyframe of configuration C
  // that has gathered matches + connections + candidates) goes through the host-driven step instead of failing the batch
  if (static_cast<int>(features.size()) > std::min(track_cap_, static_cast<int>(SDVL_MAX_ALIGN_FEATURES))) return false;
  if (t.track_.points)
    for (const shared_ptr<Point> &old : *t.track_.points) old->SetTrackRow(-1);
  const int row_base = t.track_.slot * track_cap_;
  auto table = std::make_shared<Frame::PointTable>();
  table->reserve(features.size());
  // a point may sit behind several features of a keyframe: ProjectPoints takes the first and skips the rest
  // (feature_align.cc:310: the point already carries this frame's id)
  struct Slot { Point *p; int idx; };
  static thread_local vector<Slot> hash;
  size_t hcap = 64;
  while (hcap < features.size() * 2) hcap *= 2;
  hash.assign(hcap, Slot{nullptr, -1});
  const size_t n_features = features.size();
  for (size_t fi = 0; fi < n_features; fi++) {
    // Feature -> Point -> first Feature -> keyframe: four dependent loads per row, asked for a few features ahead
    if (fi + 8 < n_features) __builtin_prefetch(features[fi + 8].get());
    if (fi + 4 < n_features && features[fi + 4]) {
      const Point *p4 = features[fi + 4]->GetPointRaw();
      __builtin_prefetch(p4);
      if (p4) __builtin_prefetch(reinterpret_cast<const char *>(p4) + 64);
    }
    if (fi + 2 < n_features && features[fi + 2]) {
      const Point *p2 = features[fi + 2]->GetPointRaw();
      if (p2) __builtin_prefetch(p2->GetInitFeatureRaw());
    }
    const shared_ptr<Feature> &ftp = features[fi];
    Feature *ft = ftp.get();
    sdvl_track_feature f;
    if (!ft) return false;
    f.px[0] = ft->GetPosition()(0); f.px[1] = ft->GetPosition()(1);
    f.bearing[0] = ft->GetVector()(0); f.bearing[1] = ft->GetVector()(1); f.bearing[2] = ft->GetVector()(2);
    f.level = ft->GetLevel();
    f.point = -1;
    Point *pt = ft->GetPointRaw();
    if (pt && !pt->ToDelete()) {
      size_t h = (reinterpret_cast<uintptr_t>(pt) >> 4) & (hcap - 1);
      while (hash[h].p && hash[h].p != pt) h = (h + 1) & (hcap - 1);
      if (hash[h].p) {
        f.point = hash[h].idx | SDVL_TRACK_DUPLICATE;
      } else {
        Feature *init = pt->GetInitFeatureRaw();
        Frame *ref = init ? init->GetFrameRaw() : nullptr;
        if (!init || !ref || ref->owner() != dev_) return false;
        const int idx = static_cast<int>(table->size());
        hash[h] = Slot{pt, idx};
        f.point = idx;
        table->push_back(ft->GetPoint());
        pt->SetTrackRow(row_base + idx);
        points->emplace_back();
        PointRow(pt, init, ref, &points->back());
        // a keyframe that never was the current frame of a tracked step (bootstrap, host-path steps): the caller registers
        // it (device calls of one context come from one thread)
        if (!ref->IsRegistered()) t.track_.up_register.push_back(ref);
      }
    }
    feats->push_back(f);
  }
  if (static_cast<int>(points->size()) > track_cap_) return false;
  t.track_.points = table;
  t.track_.stats.clear();
  t.track_.stats_dirty = false;
  return true;
}

// The points PlaneMap::SeedFromFiltered has just put on keyframe `kf` (its object features from track_.first_seed on) as table rows
// behind the rows the tables hold: point index = position in the tracker's point table, which grows by the same points.
bool SDVLBatch::AppendSeeds(SDVL &t, const shared_ptr<Frame> &kf) {
  SDVL::TrackState &ts = t.track_;
  if (!ts.points) return false;
  ts.up_points.clear();
  ts.up_feats.clear();
  const vector<shared_ptr<Feature>> &objs = kf->ObjectFeatures();
  const int row_base = ts.slot * track_cap_;
  if (static_cast<int>(ts.points->size() + (objs.size() - ts.first_seed)) > track_cap_) return false;
  if (kf->NumFlatFeatures() + static_cast<int>(objs.size()) > std::min(track_cap_, static_cast<int>(SDVL_MAX_ALIGN_FEATURES))) return false;
  if (kf->owner() != dev_ || !kf->IsRegistered()) return false;
  ts.up_points.reserve(objs.size() - ts.first_seed);
  ts.up_feats.reserve(objs.size() - ts.first_seed);
  for (size_t fi = ts.first_seed; fi < objs.size(); fi++) {
    Feature *ft = objs[fi].get();
    Point *pt = ft ? ft->GetPointRaw() : nullptr;
    if (!ft || !pt || pt->GetInitFeatureRaw() != ft) return false;  // a seed is the first observation of its own point
    sdvl_track_feature f;
    f.px[0] = ft->GetPosition()(0); f.px[1] = ft->GetPosition()(1);
    f.bearing[0] = ft->GetVector()(0); f.bearing[1] = ft->GetVector()(1); f.bearing[2] = ft->GetVector()(2);
    f.level = ft->GetLevel();
    const int idx = static_cast<int>(ts.points->size());
    f.point = idx;
    ts.points->push_back(ft->GetPoint());
    pt->SetTrackRow(row_base + idx);
    ts.up_points.emplace_back();
    PointRow(pt, ft, kf.get(), &ts.up_points.back());
    ts.up_feats.push_back(f);
  }
  return true;
}

// The rows the trackers `up` have ready (track_.up_points / up_feats) behind each other, as sdvl_track_upload / sdvl_track_append take
// them.  own_buf: for each tracker's current feature buffer (rows appended to a live table) instead of buffer 0 (a rebuilt table).
void SDVLBatch::GatherRows(const vector<int> &up, bool own_buf) {
  tr_up_points_.clear();
  tr_up_feats_.clear();
  for (vector<int32_t> *v : {&tr_up_trk_, &tr_up_buf_, &tr_up_np_, &tr_up_nf_}) v->clear();
  for (int i : up) {
    const SDVL::TrackState &ts = trk_[i]->track_;
    tr_up_trk_.push_back(i);
    tr_up_buf_.push_back(own_buf ? ts.feat_buf : 0);
    tr_up_np_.push_back(static_cast<int32_t>(ts.up_points.size()));
    tr_up_nf_.push_back(static_cast<int32_t>(ts.up_feats.size()));
    tr_up_points_.insert(tr_up_points_.end(), ts.up_points.begin(), ts.up_points.end());
    tr_up_feats_.insert(tr_up_feats_.end(), ts.up_feats.begin(), ts.up_feats.end());
  }
}

// Tables of the trackers `need` rebuilt from their last_frame's host objects and sent to the device in ONE submission.
// built == nullptr: all or nothing (false, nothing uploaded, if one of them cannot be expressed as a table);
// otherwise the expressible ones are uploaded and (*built)[q] says which.
bool SDVLBatch::UploadTables(const vector<int> &need, vector<char> *built) {
  vector<char> ok(need.size(), 0);
  ParallelFor(static_cast<int>(need.size()), [&](int q) { ok[q] = BuildTable(*trk_[need[q]]) ? 1 : 0; });
  if (!built)
    for (char o : ok)
      if (!o) return false;
  vector<int> up;
  vector<const sdvl_frame *> reg_frames;   // every reference frame the rebuilt tables name for the first time: ONE submission
  vector<double> reg_poses;
  for (size_t q = 0; q < need.size(); q++) {
    if (!ok[q]) continue;
    for (Frame *ref : trk_[need[q]]->track_.up_register)
      if (!ref->IsRegistered()) {
        double pose[7];
        ref->GetPose().ToArray(pose);
        reg_frames.push_back(ref->device());
        reg_poses.insert(reg_poses.end(), pose, pose + 7);
        ref->SetRegistered();
      }
    up.push_back(need[q]);
  }
  GatherRows(up, false);
  if (!reg_frames.empty())
    dev_->Check(sdvl_frames_register(dev_->ctx(), static_cast<int>(reg_frames.size()), reg_frames.data(), reg_poses.data()), "sdvl_frames_register");
  if (!up.empty())
    dev_->Check(sdvl_track_upload(dev_->ctx(), track_, static_cast<int>(up.size()), tr_up_trk_.data(), tr_up_buf_.data(), tr_up_np_.data(), tr_up_points_.data(),
                                  tr_up_nf_.data(), tr_up_feats_.data()), "sdvl_track_upload");
  for (int i : up) {
    trk_[i]->track_.feat_buf = 0;
    trk_[i]->track_.valid = true;
  }
  if (built) *built = ok;
  return true;
}

// ----------------------------------------------------------------------------- SDVLBatch: pieces every form of a step shares
// What the stages of one step hand to each other.
struct SDVLBatch::Step {
  Step(const vector<Image> &i, FrameStats *st, int B) : imgs(i), stats(st), decision(B, 0) {}
  const vector<Image> &imgs;
  FrameStats *stats;
  vector<shared_ptr<Frame>> frames;  // this step's frame of every tracker
  // trackers that execute ProcessFrame this step / that relocalise first / that relocalised onto a keyframe no table can express
  vector<int> run, lost, host_run;
  vector<int> init;                  // trackers in the first-frame / second-frame state of the two-frame initialisation
  vector<char> decision;             // per tracker: 0 = tracking lost / not tracked, 1 = ordinary frame, 2 = new keyframe
  vector<shared_ptr<Frame>> kfs;     // the keyframes the mapping stage seeds, and whose they are
  vector<int> kf_owner;
  bool filter_begun = false;         // FilterCornersBegin(kfs) is queued
  // the frames' corner detection is queued: set by whoever queues it first — the look-ahead of the step before (TakeLookAhead), a
  // relocalisation (Reproject searches the new frame's corners), or the step itself behind its image alignment
  bool detected = false;
  std::unique_ptr<StageClock> clk;   // the host stage the step is in
  void Stage(int id) { clk.reset(new StageClock(id)); }
  int R() const { return static_cast<int>(run.size()); }
};

// the requests of per.size() sources behind each other: (*begin)[k] = where those of source k start, the last entry = their number.
// all == nullptr: the offsets alone (the caller packs the requests itself)
static void Concatenate(const vector<vector<sdvl_search_req>> &per, vector<sdvl_search_req> *all, vector<size_t> *begin) {
  begin->resize(per.size() + 1);
  size_t total = 0;
  for (size_t k = 0; k < per.size(); k++) {
    (*begin)[k] = total;
    total += per[k].size();
    if (all) all->insert(all->end(), per[k].begin(), per[k].end());
  }
  (*begin)[per.size()] = total;
}

// The common head of a tracker's step, sdvl.cc:59-73: the new frame, and which of three states the tracker is in.  The first frame is
// saved here; what a lost and a running tracker do next is the form's business.
SDVLBatch::FrameStart SDVLBatch::BeginFrame(int i, const shared_ptr<Frame> &frame, FrameStats &st) {
  SDVL &t = *trk_[i];
  st = FrameStats();
  t.current_frame_ = frame;
  t.current_frame_->SetID(t.frame_counter_++);
  if (t.state_ != SDVL::STATE_RUNNING) {
    if (!t.two_frame_init_) t.SaveFirstFrame(st);  // otherwise InitializeTrackers, once every tracker's frame is known
    return kFirstFrame;
  }
  st.state = 2;
  return t.lost_frames_ >= 3 ? kLost : kRunning;  // relocalize = lost_frames_ >= 3, sdvl.cc:73
}

// sdvl.cc:61-71,132-177 for the trackers of the step that take the two-frame initialisation.  First-frame trackers: CreateCorners for
// 2 x NumFeatures (:135), InitFirstFrame, keyframe.  Second-frame trackers: the KLT of all of them in ONE call, then — for those whose
// shift and count pass (:234) — the RANSACs in ONE call, and per tracker the rest of ComputeHomography and InitSecondFrame.
void SDVLBatch::InitializeTrackers(Step &s) {
  vector<int> second;
  for (int i : s.init) {
    SDVL &t = *trk_[i];
    t.init_failed_ = false;
    if (t.state_ == SDVL::STATE_FIRST_FRAME) {
      if (!t.InitFirstFrame(s.stats[i])) std::cerr << "[ERROR] First frame couldn't be initialized" << std::endl;  // :138-139: stays in the state
    } else {
      second.push_back(i);
    }
  }
  if (second.empty()) return;
  // ---- TrackSecondFrame of every tracker: one sdvl_klt_track call
  vector<sdvl_klt_job> jobs(second.size());
  vector<float> prev, next;
  int at = 0;
  for (size_t k = 0; k < second.size(); k++) {
    SDVL &t = *trk_[second[k]];
    s.stats[second[k]].state = 1;
    t.h_init_->BeginSecondFrame(t.current_frame_, at, &jobs[k]);
    const int n = t.h_init_->NumPixels();
    prev.insert(prev.end(), t.h_init_->Pixels1(), t.h_init_->Pixels1() + 2 * n);
    next.insert(next.end(), t.h_init_->Pixels2(), t.h_init_->Pixels2() + 2 * n);
    at += n;
  }
  vector<uint8_t> status(std::max(at, 1));
  const sdvl_klt_params kp = {30, Config::PyramidLevels() - 1, 30, 0, 0.001, 1e-4};  // homography_init.cc:195-198
  dev_->Check(sdvl_klt_track(dev_->ctx(), static_cast<int>(jobs.size()), jobs.data(), at, prev.data(), next.data(), status.data(), nullptr, &kp),
              "sdvl_klt_track");
  vector<int> fit;  // trackers whose shift and count pass
  vector<char> done(second.size(), 0);
  for (size_t k = 0; k < second.size(); k++) {
    SDVL &t = *trk_[second[k]];
    const int n = t.h_init_->NumPixels();
    std::copy(next.begin() + 2 * jobs[k].pt_begin, next.begin() + 2 * (jobs[k].pt_begin + n), t.h_init_->Pixels2());
    if (t.h_init_->FinishTrack(status.data() + jobs[k].pt_begin)) fit.push_back(static_cast<int>(k));
  }
  // ---- cv::findHomography's RANSAC of every tracker that goes on: one sdvl_homography_ransac call
  const int max_its = 2000;
  vector<sdvl_homography_job> hjobs(fit.size());
  vector<double> src, dst;
  vector<int32_t> draws;
  int m_at = 0;
  for (size_t f = 0; f < fit.size(); f++) {
    SDVL &t = *trk_[second[fit[f]]];
    vector<double> a, b;
    vector<int32_t> d;
    t.h_init_->HomographyInput(t.rng_, max_its, &a, &b, &d);
    hjobs[f] = sdvl_homography_job{m_at, m_at + t.h_init_->NumPixels(), static_cast<int32_t>(f) * max_its, static_cast<int32_t>(f + 1) * max_its};
    src.insert(src.end(), a.begin(), a.end());
    dst.insert(dst.end(), b.begin(), b.end());
    draws.insert(draws.end(), d.begin(), d.end());
    m_at += t.h_init_->NumPixels();
  }
  if (!fit.empty()) {
    vector<sdvl_homography_result> res(fit.size());
    vector<int32_t> inl(std::max(m_at, 1));
    dev_->Check(sdvl_homography_ransac(dev_->ctx(), static_cast<int>(fit.size()), hjobs.data(), m_at, src.data(), dst.data(),
                                       static_cast<int>(fit.size()) * max_its, draws.data(), 2. / trk_[0]->camera_->GetFx(), max_its, 0.995,
                                       res.data(), inl.data()),
                "sdvl_homography_ransac");
    for (size_t f = 0; f < fit.size(); f++) {
      SDVL &t = *trk_[second[fit[f]]];
      done[fit[f]] = t.h_init_->FinishSecondFrame(res[f], inl.data() + hjobs[f].m_begin, &t.rng_) ? 1 : 0;
    }
  }
  for (size_t k = 0; k < second.size(); k++) trk_[second[k]]->SecondFrameDone(done[k] != 0, s.stats[second[k]]);
}

// Corner detection of `frames`; fork: on the context's side stream, from the caller's sdvl_ctx_fork_mark on (see SubmitTracked).
void SDVLBatch::DetectOnSideStream(const vector<shared_ptr<Frame>> &frames, bool fork) {
  if (fork) dev_->Check(sdvl_ctx_fork_begin(dev_->ctx()), "sdvl_ctx_fork_begin");
  try {
    Frame::DetectBatch(frames, Config::NumFeatures());
  } catch (...) {  // whatever the detection throws, the context leaves the fork
    if (fork) (void)sdvl_ctx_fork_end(dev_->ctx());
    throw;
  }
  if (fork) dev_->Check(sdvl_ctx_fork_end(dev_->ctx()), "sdvl_ctx_fork_end");
}

// corner counts of this step's frames (they rode along with the detection kernels: no round trip once any wait on the stream has
// returned since): the statistics need them, and with them known the keyframe round trip returns rows of exactly the right length
void SDVLBatch::FetchCornerCounts(const vector<shared_ptr<Frame>> &frames, FrameStats *stats) {
  const int B = static_cast<int>(frames.size());
  vector<sdvl_frame *> devs(B);
  vector<int32_t> counts(B);
  for (int i = 0; i < B; i++) devs[i] = frames[i]->device();
  dev_->Check(sdvl_frames_corner_counts(dev_->ctx(), B, devs.data(), counts.data()), "sdvl_frames_corner_counts");
  for (int i = 0; i < B; i++) stats[i].n_corners = counts[i];
}

// The keyframes the mapping stage will seed — what the bootstrap left pending and the fresh keyframes of plane-map trackers (other maps
// run their own mapper) — and the first half of their FilterCorners round trip (Shi-Tomasi, descriptors, one gather + copy).
// fetch_counts: FetchCornerCounts first, because it shares the context's result buffers with the round trip.
// Two callers run this early, in their pose stage, so that the bookkeeping overlaps the round trip: that work is charged to ST_MAPPING
// as well.  The epilogue, in ST_MAPPING already, runs it for the steps that could not.
void SDVLBatch::CollectKeyframes(Step &s, bool fetch_counts) {
  s.kfs.clear();
  s.kf_owner.clear();
  for (size_t i = 0; i < trk_.size(); i++) {
    const bool fresh = s.decision[i] == 2 && !dynamic_cast<MapperMap *>(trk_[i]->map_);
    if (trk_[i]->pending_kf_) { s.kfs.push_back(trk_[i]->pending_kf_); s.kf_owner.push_back(static_cast<int>(i)); }
    else if (fresh) { s.kfs.push_back(trk_[i]->current_frame_); s.kf_owner.push_back(static_cast<int>(i)); }
  }
  if (s.kfs.empty()) return;
  std::unique_ptr<StageClock> nested(s.clk->id != ST_MAPPING ? new StageClock(ST_MAPPING) : nullptr);
  if (fetch_counts) FetchCornerCounts(s.frames, s.stats);
  Frame::FilterCornersBegin(s.kfs);
  s.filter_begun = true;
}

// -------------------------------------------------------------------------------- SDVLBatch: relocalisation inside the tabled step
static std::atomic<unsigned long long> g_reloc_epoch{1};  // process-wide: a cache never mistakes another batch's store for its own

// The alignments of RelocalizeLost: jobs whose feature ranges name records of the batch's store, in launches of bounded size
// (a farm whose trackers are all lost asks for B x |keyframes| alignments per step).
void SDVLBatch::RelocAlign(const vector<sdvl_align_job> &jobs, const sdvl_align_params &ap, vector<sdvl_align_result> *res) {
  res->resize(jobs.size());
  const sdvl_camera cam = trk_[0]->camera_->abi();
  const size_t kChunk = 4096;
  for (size_t b = 0; b < jobs.size(); b += kChunk) {
    const int n = static_cast<int>(std::min(jobs.size(), b + kChunk) - b);
    dev_->Check(sdvl_image_align_begin_stored(dev_->ctx(), n, jobs.data() + b, reloc_store_, &cam, &ap), "sdvl_image_align_begin_stored");
    dev_->Check(sdvl_image_align_end(dev_->ctx(), n, res->data() + b), "sdvl_image_align_end");
  }
}

// t.reloc_ of the keyframes of t's map, newest first (the order Relocalize visits them in); their feature records go behind *packed
void SDVLBatch::PackRelocCache(SDVL &t, vector<sdvl_align_feature> *packed) {
  SDVL::RelocCache &rc = t.reloc_;
  rc.kfs.clear();
  rc.begin.assign(1, 0);
  rc.T.clear();
  vector<shared_ptr<Frame>> &kfs = t.map_->GetKeyframes();
  for (auto it = kfs.rbegin(); it != kfs.rend(); it++) {
    rc.kfs.push_back(*it);
    // (a keyframe holds its matches plus at most one seed per free grid cell, and the seeds are filtered corners: <= max_matches +
    // num_features whatever the grid, 1200 with the TUM settings even on 8160 cells; a keyframe beyond SDVL_MAX_ALIGN_FEATURES (2048)
    // makes the stored alignment report SDVL_ERR_CAPACITY, at any frame size)
    ImageAlign::PackFeatures(**it, packed);
    rc.begin.push_back(static_cast<int32_t>(packed->size()));
    double T7[7];
    ((*it)->GetPose() * (*it)->GetPose().Inverse()).ToArray(T7);  // current_frame_->SetPose(cframe->GetPose()), then image_align.cc:66
    rc.T.insert(rc.T.end(), T7, T7 + 7);
  }
}

// The keyframes' feature records of the trackers `lost`: they do not change while a tracker is lost (no tracked step, the mapper stands
// still), so they are packed once and stay in HBM (sdvl_align_store; SDVL::RelocCache remembers where) — packed again only for the
// trackers whose map changed since, or that were not lost before.  Per frame only the job records cross the link.
void SDVLBatch::RefreshRelocStore(const vector<int> &lost) {
  const int L = static_cast<int>(lost.size());
  vector<vector<sdvl_align_feature>> fresh(L);
  vector<char> stale(L, 0);
  for (int q = 0; q < L; q++) {
    SDVL &t = *trk_[lost[q]];
    SyncStats(t);  // the Point objects Reproject reads catch up with the device's counters
    t.StartRelocalizing();
    const SDVL::RelocCache &rc = t.reloc_;
    stale[q] = (!reloc_store_ || rc.owner != this || rc.epoch != reloc_epoch_ || rc.version != t.map_->Version()) ? 1 : 0;
  }
  ParallelFor(L, [&](int q) {
    if (stale[q]) PackRelocCache(*trk_[lost[q]], &fresh[q]);
  });
  size_t need = 0;
  for (int q = 0; q < L; q++)
    if (stale[q]) need += fresh[q].size();
  if (need == 0) return;  // also when every keyframe is empty — with no store yet none is made, and RelocAlign meets a null one
  if (!reloc_store_ || reloc_used_ + need > static_cast<size_t>(reloc_cap_)) {
    // no room behind the records in use: a new store for what is live now (the other trackers' caches are void: epoch)
    size_t live = need;
    for (int q = 0; q < L; q++)
      if (!stale[q]) {
        stale[q] = 1;  // repack: its records die with the old store
        PackRelocCache(*trk_[lost[q]], &fresh[q]);
        live += fresh[q].size();
      }
    if (reloc_store_) dev_->Check(sdvl_align_store_destroy(dev_->ctx(), reloc_store_), "sdvl_align_store_destroy");
    reloc_store_ = nullptr;
    reloc_epoch_ = g_reloc_epoch++;
    reloc_used_ = 0;
    const size_t cap = std::max<size_t>(2 * live, 65536);
    if (cap > 0x7fffffffu) throw std::runtime_error("SDVLBatch: relocalisation store too large");
    dev_->Check(sdvl_align_store_create(dev_->ctx(), static_cast<int>(cap), &reloc_store_), "sdvl_align_store_create");
    reloc_cap_ = static_cast<int>(cap);
  }
  vector<sdvl_align_feature> all;
  const int base = reloc_used_;
  for (int q = 0; q < L; q++) {
    if (!stale[q]) continue;
    SDVL &t = *trk_[lost[q]];
    SDVL::RelocCache &rc = t.reloc_;
    const int32_t off = base + static_cast<int32_t>(all.size());
    for (int32_t &b : rc.begin) b += off;
    all.insert(all.end(), fresh[q].begin(), fresh[q].end());
    rc.owner = this;
    rc.epoch = reloc_epoch_;
    rc.version = t.map_->Version();
  }
  dev_->Check(sdvl_align_store_write(dev_->ctx(), reloc_store_, base, static_cast<int>(all.size()), all.data()), "sdvl_align_store_write");
  reloc_used_ = base + static_cast<int>(all.size());
}

// The alignment of every lost tracker's current frame against EVERY keyframe of its map (each started from that keyframe's pose, fast
// mode): independent of each other, one launch for all (tracker, keyframe) pairs.  (*first)[q] = the first job of tracker lost[q].
// Fast mode gives up behind the coarsest level when the update there is still > 0.01 (image_align.cc:73-76), and on a frame that shows
// something else nearly every keyframe does: the launch runs that level ONLY (a third of PrecomputePatches); the few jobs that pass it
// are run again in full — same start, same arithmetic, so both passes leave what one full pass would.
void SDVLBatch::RelocAlignKeyframes(const vector<int> &lost, vector<int> *first, vector<sdvl_align_result> *res) {
  const int L = static_cast<int>(lost.size());
  vector<sdvl_align_job> jobs;
  first->assign(L + 1, 0);
  for (int q = 0; q < L; q++) {
    SDVL &t = *trk_[lost[q]];
    const SDVL::RelocCache &rc = t.reloc_;
    (*first)[q] = static_cast<int>(jobs.size());
    for (size_t j = 0; j < rc.kfs.size(); j++) {
      if (rc.begin[j + 1] == rc.begin[j]) std::cerr << "[ERROR] No points to track!" << std::endl;  // image_align.cc:55-58
      sdvl_align_job jb;
      jb.ref = rc.kfs[j]->device();
      jb.cur = t.current_frame_->device();
      jb.feat_begin = rc.begin[j];
      jb.feat_end = rc.begin[j + 1];
      std::memcpy(jb.T, rc.T.data() + 7 * j, sizeof(jb.T));
      jobs.push_back(jb);
    }
  }
  (*first)[L] = static_cast<int>(jobs.size());
  if (jobs.empty()) return;
  sdvl_align_params ap = AlignParams(true);
  const int min_level = ap.min_level;
  ap.min_level = ap.max_level;  // the coarsest level alone
  RelocAlign(jobs, ap, res);
  if (min_level >= ap.max_level) return;
  vector<int> pass;
  for (size_t j = 0; j < jobs.size(); j++)
    if ((*res)[j].error <= 0.01) pass.push_back(static_cast<int>(j));  // image_align.cc:73-76 did not give up: the finer levels follow
  if (pass.empty()) return;
  vector<sdvl_align_job> again;
  for (int j : pass) again.push_back(jobs[j]);
  vector<sdvl_align_result> full;
  ap.min_level = min_level;
  RelocAlign(again, ap, &full);
  for (size_t k = 0; k < pass.size(); k++) (*res)[pass[k]] = full[k];
}

// SDVL::Relocalize (sdvl.cc:73-89,205-238) for the trackers `lost` of a batch, inside the tabled step: the other trackers of the batch
// are not touched.  (*found)[q]: tracker lost[q] has relocalised — last_frame_ = last_kf_ = the keyframe it landed on (sdvl.cc:84-86).
// The keyframe loop, sdvl.cc:209-235, runs over the alignments' results in the reference's order (newest first).  Reproject(reloc = true)
// draws from rand() and stops at the first keyframe that gathers MinMatches, so it stays sequential per tracker — but the trackers
// advance together: one search launch per ROUND (a round = every unresolved tracker's next keyframe with error < 0.001; almost always
// there is one round).
void SDVLBatch::RelocalizeLost(const vector<int> &lost, FrameStats *stats, vector<char> *found) {
  found->assign(lost.size(), 0);
  RefreshRelocStore(lost);
  vector<int> first;
  vector<sdvl_align_result> res;
  RelocAlignKeyframes(lost, &first, &res);
  const int L = static_cast<int>(lost.size());
  vector<int> cursor(first.begin(), first.end() - 1);
  vector<char> open_(L, 1);
  vector<vector<sdvl_search_req>> per(L);
  vector<sdvl_search_req> reqs;
  vector<sdvl_search_res> sres;
  vector<size_t> begin(L + 1, 0);
  for (;;) {
    bool any = false;
    reqs.clear();
    for (int q = 0; q < L; q++) {
      per[q].clear();
      if (!open_[q]) continue;
      SDVL &t = *trk_[lost[q]];
      const SDVL::RelocCache &rc = t.reloc_;
      // every keyframe visited leaves its aligned pose on the frame (image_align.cc:79); those with error >= 0.001 are passed over
      while (cursor[q] < first[q + 1]) {
        const int j = cursor[q] - first[q];
        if (rc.begin[j + 1] > rc.begin[j])  // (ComputePose returns before touching the pose when frame1 has no features)
          t.current_frame_->SetPose(SE3::FromArray(res[cursor[q]].T) * rc.kfs[j]->GetPose());
        else
          t.current_frame_->SetPose(rc.kfs[j]->GetPose());
        const double err = rc.begin[j + 1] > rc.begin[j] ? res[cursor[q]].error : 1e10;
        if (err < 0.001) break;
        cursor[q]++;
      }
      if (cursor[q] >= first[q + 1]) {
        open_[q] = 0;
        continue;
      }
      const shared_ptr<Frame> &cframe = rc.kfs[cursor[q] - first[q]];
      t.feature_align_.PrepareReproject(t.current_frame_, cframe, true, &per[q]);
      any = true;
    }
    if (!any) break;
    Concatenate(per, &reqs, &begin);
    Matcher::SearchPoints(dev_, reqs, *trk_[lost[0]]->camera_, &sres);
    for (int q = 0; q < L; q++) {
      if (!open_[q] || cursor[q] >= first[q + 1]) continue;
      SDVL &t = *trk_[lost[q]];
      t.feature_align_.FinishReproject(t.current_frame_, sres.data() + begin[q]);
      t.matches_ = t.feature_align_.GetMatches();
      t.attempts_ = t.feature_align_.GetAttempts();
      if (t.matches_ >= Config::MinMatches()) {
        t.Relocalized(t.reloc_.kfs[cursor[q] - first[q]], stats[lost[q]]);
        (*found)[q] = 1;
        open_[q] = 0;
      } else {
        cursor[q]++;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------- SDVLBatch: the step on the tables
// ProcessFrame (sdvl.cc:179-203) of ONE tracker through the per-object calls (ImageAlign::ComputePose, FeatureAlign::Reproject /
// OptimizePose), inside a tabled step: for the tracker whose last_frame no table can express (a keyframe with more features than the
// alignment kernels take) while everybody else stays on the tables.  Returns the decision (0 lost, 1 frame, 2 keyframe).
int SDVLBatch::TrackOnHost(SDVL &t, FrameStats *st) {
  st->host_path = 2;
  ImageAlign image_align;
  st->align_meas = image_align.ComputePose(t.last_frame_, t.current_frame_);
  st->align_features = static_cast<int>(t.last_frame_->GetFeatures().size());
  t.feature_align_.Reproject(t.current_frame_, t.last_frame_, t.last_kf_);
  t.matches_ = t.feature_align_.GetMatches();
  t.attempts_ = t.feature_align_.GetAttempts();
  t.feature_align_.OptimizePose(t.current_frame_);
  st->inliers = t.feature_align_.GetInliers();
  st->outliers = t.feature_align_.GetOutliers();
  t.GetMotionModel();
  t.track_.valid = false;  // this frame's features live on the host
  return t.TrackingDecision();
}

// Whether the batch can step on the tables at all.  The rows of a tracker's table live in the set of ONE batch: a tracker that was last
// stepped by another batch (a farm batch and its own SDVL::HandleFrame batch, say) brings its counters up to date and gets its table
// rebuilt, under this batch's slot.
bool SDVLBatch::TrackedStepApplies() {
  if (!TrackTables() || !DevicePose() || Config::MaxRansacPoints() > 8) return false;
  for (SDVL *t : trk_) {
    if (t->feature_align_.MaxMatches() > FeatureAlign::kMaxDevicePoseObs || t->feature_align_.MaxMatches() < 1) return false;
    if (t->camera_ != trk_[0]->camera_) return false;
  }
  for (size_t i = 0; i < trk_.size(); i++) {
    SDVL::TrackState &ts = trk_[i]->track_;
    if (ts.owner != this) {
      SyncStats(*trk_[i]);
      ts.valid = false;
      ts.append_pending = false;
      ts.owner = this;
    }
    ts.slot = static_cast<int>(i);
  }
  return true;
}

// the set of tables, made at the first tracked step; false: the detection grid is one the set cannot serve
bool SDVLBatch::EnsureTrackSet() {
  const int cells = trk_[0]->feature_align_.GridCells();
  if (cells > 65535) return false;
  if (!track_) {
    // a keyframe holds its matches plus what the mapper adds (one seed per free grid cell with the plane map): twice that
    // leaves room for the reference mapper's connection points; a frame that outgrows it is tracked on the host path
    int mm = 1;
    for (SDVL *t : trk_) mm = std::max(mm, t->feature_align_.MaxMatches());
    // (large grids, e.g. 8160 cells at 3840x2160 / 32: the cap stays 4096 rows; a keyframe with more goes to the host path)
    track_cap_ = std::min(4096, 2 * (mm + cells));
    track_cells_ = cells;
    dev_->Check(sdvl_track_create(dev_->ctx(), static_cast<int>(trk_.size()), track_cap_, track_cap_, cells, mm, Config::MaxRansacIts(), &track_),
                "sdvl_track_create");
  }
  return cells == track_cells_;
}

// the frames of a look-ahead (SetNextImages before the previous step): pyramids and detection are queued already
void SDVLBatch::TakeLookAhead(Step &s) {
  if (ahead_frames_.empty()) return;
  const size_t B = trk_.size();
  bool same = ahead_frames_.size() == B && s.imgs.size() == B;
  for (size_t i = 0; same && i < B; i++) same = s.imgs[i].dev_src != nullptr && s.imgs[i].dev_src == ahead_src_[i];
  if (same) {
    s.frames.swap(ahead_frames_);
    s.detected = true;
  }
  ahead_frames_.clear();
  ahead_src_.clear();
}

// the look-ahead: the next step's pyramids and detection go behind this step's chain, ahead of its keyframe kernels
void SDVLBatch::QueueLookAhead(const Step &s) {
  const size_t B = trk_.size();
  if (next_imgs_.empty() || s.run.size() != B || next_imgs_.size() != B) return;
  bool device_images = true;
  for (const Image &im : next_imgs_) device_images = device_images && im.dev_src != nullptr && !im.transient;
  if (!device_images) return;
  Frame::CreateBatch(trk_[0]->camera_, &trk_[0]->orb_detector_, next_imgs_, false, Config::NumFeatures(), &ahead_frames_, &pfor_);
  Frame::DetectBatch(ahead_frames_, Config::NumFeatures());
  ahead_src_.clear();
  for (const Image &im : next_imgs_) ahead_src_.push_back(im.dev_src);
}

// Relocalize for the trackers that lost their map, in THIS step: their alignments and searches are extra launches of the same
// submission queue; the trackers that found a keyframe join the tracked step with a table built from that keyframe (ProcessFrame(
// last_frame_ = last_kf_ = the keyframe), sdvl.cc:86-93), the others sit this frame out (sdvl.cc:91: !relocalize).
void SDVLBatch::RelocalizeIntoStep(Step &s) {
  s.Stage(ST_RELOCALIZE);
  if (!s.detected) {  // Reproject searches the new frame's corners
    Frame::DetectBatch(s.frames, Config::NumFeatures());
    s.detected = true;
  }
  vector<char> found;
  RelocalizeLost(s.lost, s.stats, &found);
  vector<int> again;
  for (size_t q = 0; q < s.lost.size(); q++)
    if (found[q]) again.push_back(s.lost[q]);
  if (!again.empty()) {
    vector<char> built;
    UploadTables(again, &built);
    for (size_t q = 0; q < again.size(); q++) {
      trk_[again[q]]->SetMotionModel();  // (vel_ = 0)
      (built[q] ? s.run : s.host_run).push_back(again[q]);
    }
    std::sort(s.run.begin(), s.run.end());
  }
  s.Stage(ST_PRELUDE);
}

// the step's inputs: jobs, the cell order SelectPoints would shuffle (feature_align.cc:103), the draws SelectInliers would make
sdvl_track_params SDVLBatch::AssembleTrackJobs(const Step &s) {
  const int R = s.R(), cells = track_cells_, max_its = Config::MaxRansacIts();
  tr_jobs_.resize(R);
  tr_rank_.resize(static_cast<size_t>(R) * cells);
  tr_rand_.resize(static_cast<size_t>(R) * max_its);
  ParallelFor(R, [&](int k) {
    SDVL &t = *trk_[s.run[k]];
    sdvl_track_job &jb = tr_jobs_[k];
    jb.tracker = s.run[k];
    jb.feat_buf = t.track_.feat_buf;
    jb.last = t.last_frame_->device();
    jb.cur = t.current_frame_->device();
    const SE3 T = t.current_frame_->GetPose() * t.last_frame_->GetPose().Inverse();  // image_align.cc:66
    T.ToArray(jb.T);
    t.last_frame_->GetPose().ToArray(jb.last_pose);
    jb.frame_id = t.current_frame_->GetID();
    jb.max_matches = t.feature_align_.MaxMatches();
    t.feature_align_.ShuffleCellRanks(tr_rank_.data() + static_cast<size_t>(k) * cells);
    t.feature_align_.PeekRand(max_its, tr_rand_.data() + static_cast<size_t>(k) * max_its);
  });
  sdvl_track_params prm;
  prm.align = AlignParams(false);
  prm.search = SearchParams();
  prm.pose = FeatureAlign::PoseParams(*trk_[0]->camera_);
  prm.cell_size = Config::CellSize();
  prm.patch_size = Config::PatchSize();
  prm.max_failed = Config::MaxFailed();
  prm.pad_ = 0;
  return prm;
}

// the step of the trackers s.run: ONE submission (alignment, detection, reprojection, search, match selection, pose, table update), ONE wait
void SDVLBatch::SubmitTracked(Step &s) {
  const int R = s.R();
  s.Stage(ST_IMAGE_ALIGN);
  const sdvl_track_params prm = AssembleTrackJobs(s);
  const sdvl_camera cam = trk_[0]->camera_->abi();
  // A SMALL batch (a lone camera's HandleFrame above all) is a chain of launches that each fill a sliver of the chip: its detection
  // (FAST, selection: needs the pyramid only) runs on the context's side stream BESIDE the alignment instead of behind it
  // (sdvl_ctx_fork_*); a farm's batches keep one stream per group — there the other groups are the company, and a whole-context wait
  // inside a fork would block the worker's other groups (B <= 4: the batches that also spin on their waits).
  const bool fork = !s.detected && trk_.size() <= 4;
  if (fork) dev_->Check(sdvl_ctx_fork_mark(dev_->ctx()), "sdvl_ctx_fork_mark");  // the pyramids are queued: the side chain starts here
  dev_->Check(sdvl_track_align(dev_->ctx(), track_, R, tr_jobs_.data(), tr_rank_.data(), tr_rand_.data(), &cam, &prm), "sdvl_track_align");
  if (!s.detected) {
    DetectOnSideStream(s.frames, fork);  // (no fork: FAST + selection run behind the alignment)
    s.detected = true;
  }
  s.Stage(ST_SEARCH);
  dev_->Check(sdvl_track_search(dev_->ctx(), track_), "sdvl_track_search");
  QueueLookAhead(s);
  tr_res_.resize(R);
  dev_->Check(sdvl_track_collect(dev_->ctx(), track_, R, tr_res_.data()), "sdvl_track_collect");
}

// the step's results: pose, counters, the rand() stream, deletions, motion model, tracking quality, keyframe decision
void SDVLBatch::ReplayTracked(Step &s) {
  const int R = s.R();
  s.Stage(ST_FINISH);
  for (int k = 0; k < R; k++)
    if (tr_res_[k].status != 0) throw std::runtime_error("sdvl_track: a table capacity was exceeded on the device");
  ParallelFor(R, [&](int k) {
    const int i = s.run[k];
    SDVL &t = *trk_[i];
    FrameStats &st = s.stats[i];
    const sdvl_track_result &r = tr_res_[k];
    SDVL::TrackState &ts = t.track_;
    st.align_meas = r.align_meas;
    st.align_iters = r.align_iters;
    st.align_features = r.n_features;
    st.search_requests = r.n_requests;
    st.lk_iters = r.lk_iters;
    st.n_corners = r.n_corners;
    t.current_frame_->SetPose(SE3::FromArray(r.pose));
    t.current_frame_->SetRegistered();  // the step wrote (view, final pose) into the registry
    t.current_frame_->SetFlatFeatures(sdvl_track_features(track_, k), r.matches, ts.points);
    t.current_frame_->SetSceneDepthHint(r.scene_depth);
    const sdvl_track_point_stat *ps = sdvl_track_stats(track_, k);
    ts.stats.assign(ps, ps + ts.points->size());
    ts.stats_dirty = true;
    if (dynamic_cast<MapperMap *>(t.map_)) SyncStats(t);  // the mapper's depth filter reads and resets the failure counts
    t.feature_align_.AdvanceRand(r.n_draws);
    t.feature_align_.SetTrackedCounts(r.matches, r.attempts, r.n_inliers, r.n_outliers);
    t.matches_ = r.matches;
    t.attempts_ = r.attempts;
    st.inliers = r.n_inliers;
    st.outliers = r.n_outliers;
    if (r.n_deleted > 0)  // points that crossed MaxFailed: Map::DeletePoint (feature_align.cc:141-142), emptied in the epilogue
      for (size_t p = 0; p < ts.points->size(); p++)
        if ((ts.stats[p].status & 0x100) && !(*ts.points)[p]->ToDelete()) {
          (*ts.points)[p]->SetDeviceTrashed();  // the row carries the deletion: nothing to rebuild when the trash is emptied
          t.map_->DeletePoint((*ts.points)[p]);
        }
    t.GetMotionModel();
    s.decision[i] = static_cast<char>(t.TrackingDecision());
  });
}

// What the decisions set off, sdvl.cc:101-121, for every tracker that executed ProcessFrame this step.  (Charged to ST_POSE.)
void SDVLBatch::SaveTrackedFrames(Step &s) {
  vector<int> act(s.run);
  act.insert(act.end(), s.host_run.begin(), s.host_run.end());
  if (act.empty()) return;
  s.Stage(ST_POSE);
  // the keyframes are known: queue their FilterCorners inputs now; the bookkeeping below runs meanwhile.  The counts of bootstrap
  // frames and of trackers that sat the step out or were tracked by hand did not ride along with the step's results: fetched first.
  CollectKeyframes(s, s.run.size() < trk_.size());
  vector<int> r_matches(trk_.size(), 0);
  for (size_t k = 0; k < s.run.size(); k++) r_matches[s.run[k]] = tr_res_[k].matches;
  ParallelFor(static_cast<int>(act.size()), [&](int a) {
    const int i = act[a];
    SDVL &t = *trk_[i];
    if (s.decision[i] == 0) return;  // tracking lost: last_frame and its table stay
    if (s.decision[i] == 2) {
      // Plane-map trackers: the keyframe's matched features STAY flat records and its table stays the one the step has just left on
      // the device — the points the map seeds in its empty cells are appended to both sides after the seeding (FinishKeyframes ->
      // AppendSeeds -> sdvl_track_append).  The objects appear the first time somebody asks (Frame::GetFeatures()).
      const bool plane = !dynamic_cast<MapperMap *>(t.map_);
      const size_t rows = t.track_.points ? t.track_.points->size() : static_cast<size_t>(track_cap_);
      const bool room = static_cast<int>(rows) + track_cells_ <= track_cap_ && r_matches[i] + track_cells_ <= track_cap_;
      if (plane && room && t.current_frame_->HasFlatFeatures()) {
        t.current_frame_->LinkPointsOnMaterialize();
        t.track_.feat_buf ^= 1;  // the matches the step left in the other buffer are last_frame's features now
        t.track_.append_pending = true;
        t.track_.first_seed = t.current_frame_->ObjectFeatures().size();
      } else {
        // the frame becomes part of the map: its features and the points behind them turn into objects
        SyncStats(t);
        t.LinkFeatures();
        t.track_.valid = false;  // seeding / the mapper add features: the table is rebuilt from the keyframe
      }
      t.current_frame_->ClearSceneDepthHint();  // a keyframe's features lose the points EmptyTrash deletes (map.cc:207-259)
      t.SaveKeyframe(s.stats[i]);
    } else {
      t.map_->AddFrame(t.current_frame_);
      if (t.current_frame_->HasFlatFeatures()) t.track_.feat_buf ^= 1;  // the matches the step left in the other buffer are last_frame's features now
    }
    t.last_frame_ = t.current_frame_;
  });
}

// With the reference's mapper the tracker follows CANDIDATES too (Map::InitCandidates links them to the keyframe at once,
// map.cc:379-390), and the depth filter rewrites their inverse depth, variance, position, failure count and finally
// `fixed` after every frame (point.cc:64-100,164-178).  With the filter on the device (depth_filter_kernel) the rows are
// patched where they lie, in the same stream, and the table stays valid; it is rebuilt from the objects when the filter ran
// on the host or on another context (threaded mode), and whenever a point with a row died behind the device's back.
void SDVLBatch::InvalidateStaleTables() {
  for (SDVL *tp : trk_) {
    SDVL &t = *tp;
    MapperMap *m = dynamic_cast<MapperMap *>(t.map_);
    if (m && (m->IsThreaded() || !MapperMap::DeviceFilter())) t.track_.valid = false;
    if (t.map_->TakeTablesDirty()) t.track_.valid = false;
    // tracking lost: last_frame stays, but the mapper has had it and trashed it — its features are gone from the host
    // (MapperMap::EmptyTrash, map.cc:207-259) and the next step must not find them in the table either
    if (t.last_frame_ && t.last_frame_->FeaturesRemoved()) t.track_.valid = false;
  }
}

// One step of B trackers on the device-resident tables.  The host keeps what only it can do: rand() (cell shuffle, RANSAC draws), the
// motion model, tracking quality, the keyframe decision and everything a keyframe sets off.  false: not applicable this step.
bool SDVLBatch::HandleFramesTracked(const vector<Image> &imgs, FrameStats *stats) {
  if (!TrackedStepApplies() || !EnsureTrackSet()) return false;
  const int B = static_cast<int>(trk_.size());
  Step s(imgs, stats, B);
  // ---- tables of the trackers whose last_frame changed behind the device's back (keyframes: seeded / mapped features).  First of all: a
  // frame no table can express sends the whole step to the host path, untouched.  (A relocalising tracker gets its table further down.)
  s.Stage(ST_PREPARE);
  vector<int> need;
  for (int i = 0; i < B; i++)
    if (trk_[i]->state_ == SDVL::STATE_RUNNING && !trk_[i]->track_.valid && trk_[i]->lost_frames_ < 3) need.push_back(i);
  if (!need.empty() && !UploadTables(need, nullptr)) return false;
  // ---- stage 0: Frame construction, sdvl.cc:59 (pyramids now, detection behind the alignment)
  TakeLookAhead(s);
  if (!s.detected) Frame::CreateBatch(trk_[0]->camera_, &trk_[0]->orb_detector_, imgs, false, Config::NumFeatures(), &s.frames, &pfor_);
  s.Stage(ST_PRELUDE);
  for (int i = 0; i < B; i++) {
    const FrameStart start = BeginFrame(i, s.frames[i], stats[i]);
    if (start == kLost) s.lost.push_back(i);
    if (start == kFirstFrame && trk_[i]->two_frame_init_) s.init.push_back(i);
    if (start != kRunning) continue;
    trk_[i]->SetMotionModel();
    s.run.push_back(i);
  }
  if (!s.init.empty()) InitializeTrackers(s);
  if (!s.lost.empty()) RelocalizeIntoStep(s);
  if (!s.run.empty()) {
    SubmitTracked(s);
    ReplayTracked(s);
  }
  // (a relocalised tracker whose keyframe no table can hold: the per-object calls, behind the batch's chain on the same stream)
  for (int i : s.host_run) s.decision[i] = static_cast<char>(TrackOnHost(*trk_[i], &stats[i]));
  SaveTrackedFrames(s);
  s.clk.reset();
  next_imgs_.clear();  // a look-ahead belongs to ONE step, whether that step could use it (every tracker tracked) or not (bootstrap)
  if (s.run.empty() && !s.detected) {  // bootstrap-only step: the new keyframes still need their corners
    // (a small batch detects on the side stream here too: the stream and its queue exist by the time a tracked frame forks)
    const bool fork = B <= 4;
    if (fork) dev_->Check(sdvl_ctx_fork_mark(dev_->ctx()), "sdvl_ctx_fork_mark");
    DetectOnSideStream(s.frames, fork);
  }
  // a mapper that looks at the frames it was given (MapperMap: scene depth of every frame, feature lists of keyframes)
  // materialises them on demand; a keyframe's table is rebuilt afterwards in any case
  EpilogueAndMapper(s);
  InvalidateStaleTables();
  return true;
}

// SDVL::HandleFrame (sdvl.cc:55-130) for B trackers
void SDVLBatch::HandleFrames(const vector<Image> &imgs, FrameStats *stats) {
  const int B = static_cast<int>(trk_.size());
  if (static_cast<int>(imgs.size()) != B) throw std::runtime_error("SDVLBatch::HandleFrames: one image per tracker");
  Device::SetCurrent(dev_);
  StageTimes::Active() = &stage_times;
  stage_times.steps++;
  const auto t_begin = std::chrono::steady_clock::now();
  // A transient image (level 0 aliases a ring slot the caller rewrites) is safe only while nobody reads a frame's level 0 after
  // the frame's own step.  Two configurations break that:
  //  * a mapper THREAD consumes the frames handed to AddFrame after the step, on its own stream: such a batch takes a copy of
  //    every image when the frame is built (the aliasing is refused);
  //  * SDVL.min_alignLevel 0: the next step's image alignment reads last_frame's level 0 (image_align.cc:212): last_frame copies
  //    its image out at the end of the step like a fresh keyframe does.
  bool threaded_mapper = false;
  for (SDVL *t : trk_) {
    MapperMap *m = dynamic_cast<MapperMap *>(t->map_);
    if (m && m->IsThreaded()) threaded_mapper = true;
  }
  vector<Image> owned;
  if (threaded_mapper && std::any_of(imgs.begin(), imgs.end(), [](const Image &im) { return im.transient; })) {
    owned = imgs;
    for (Image &im : owned)
      if (im.transient) { im.transient = false; im.borrow = false; }
  }
  const vector<Image> &in = owned.empty() ? imgs : owned;
  if (!HandleFramesTracked(in, stats)) {
    next_imgs_.clear();  // the host-driven path takes no look-ahead, and one that was queued is dropped
    ahead_frames_.clear();
    ahead_src_.clear();
    SyncHostState();  // Feature lists and Point counters catch up with the device; the tables are rebuilt when tracking returns
    HandleFramesGeneric(in, stats);
  }
  {  // frames that became keyframes while their image sat in an input-ring slot keep a copy; everybody else never copied level 0
     // (the step's own frame pointer is gone by now: a fresh keyframe is the tracker's last_kf_, sdvl.cc:113)
    const bool keep_last = Config::MinAlignLevel() == 0;
    vector<shared_ptr<Frame>> keep;
    for (SDVL *t : trk_) {
      if (t->last_kf_ && t->last_kf_->ImageTransient()) keep.push_back(t->last_kf_);
      if (keep_last && t->last_frame_ && t->last_frame_ != t->last_kf_ && t->last_frame_->ImageTransient()) keep.push_back(t->last_frame_);
    }
    if (!keep.empty()) Frame::OwnImages(keep);
  }
  stage_times.t[ST_TOTAL] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  StageTimes::Active() = nullptr;
}

// ------------------------------------------------------------------------------------------ SDVLBatch: the host-driven step
// what the stages of the host-driven form hand to each other on top of Step; index k = position in `run`
struct SDVLBatch::HostStep : SDVLBatch::Step {
  HostStep(const vector<Image> &i, FrameStats *st, int B) : Step(i, st, B), device_pose(DevicePose()) {}
  const bool device_pose;
  // the search requests: in the pinned staging area of one search batch (packed), with the pose stage behind them in the same submission
  // (chain), or in scratch_reqs_; those of run[k] are [begin[k], begin[k + 1])
  bool packed = false, chain = false;
  FeatureAlign::PackedSink sink;
  vector<size_t> begin;
  vector<sdvl_chain_frame> chain_frames;
  vector<int> chain_obs_begin;
  vector<sdvl_search_res> res;
  // the pose jobs: per tracker with several host threads, else straight into scratch_pose_; job_of[k] = its job there or -1 (host pose)
  vector<FeatureAlign::PoseBatch> pb;
  vector<int> job_of;
  vector<char> on_device;
  vector<sdvl_pose_result> pres;
  vector<int32_t> lists;
};

// Relocalize, sdvl.cc:73-89,205-238, for one tracker.  The alignment of the current frame against EVERY keyframe (each started
// from that keyframe's pose, fast mode) is independent of the others: one launch with |keyframes| jobs.  The keyframe loop then
// runs in the reference's order (newest first) over the results; Reproject stays sequential because it draws from rand() and
// stops at the first keyframe that gathers MinMatches.  true: relocalised.
bool SDVLBatch::RelocalizeOnHost(SDVL &t, FrameStats &st) {
  t.StartRelocalizing();
  vector<shared_ptr<Frame>> &kfs = t.map_->GetKeyframes();
  vector<std::pair<shared_ptr<Frame>, shared_ptr<Frame>>> pairs;
  vector<SE3> start, aligned;
  for (auto it = kfs.rbegin(); it != kfs.rend(); it++) {
    pairs.push_back({*it, t.current_frame_});
    start.push_back((*it)->GetPose());
  }
  vector<int> n_meas;
  vector<double> errors;
  ImageAlign::ComputePoseBatch(pairs, true, &n_meas, &errors, nullptr, &start, &aligned);
  for (size_t j = 0; j < pairs.size(); j++) {
    const shared_ptr<Frame> &cframe = pairs[j].first;
    t.current_frame_->SetPose(aligned[j]);
    if (errors[j] >= 0.001) continue;
    t.feature_align_.Reproject(t.current_frame_, cframe, cframe, true);
    t.matches_ = t.feature_align_.GetMatches();
    t.attempts_ = t.feature_align_.GetAttempts();
    if (t.matches_ >= Config::MinMatches()) {
      t.Relocalized(cframe, st);
      return true;
    }
  }
  return false;
}

// stage 1: ImageAlign for every running tracker, sdvl.cc:185-190.  FAST + selection + ORB are queued BEHIND the alignment, which only
// needs the pyramids: its results reach the host earlier and detection overlaps the host's prepare stage
void SDVLBatch::AlignImages(HostStep &s) {
  s.Stage(ST_IMAGE_ALIGN);
  vector<std::pair<shared_ptr<Frame>, shared_ptr<Frame>>> pairs;
  for (int i : s.run) pairs.push_back({trk_[i]->last_frame_, trk_[i]->current_frame_});
  vector<int> n_meas, iters;
  vector<double> errors;
  const std::function<void()> detect = [&]() { Frame::DetectBatch(s.frames, Config::NumFeatures()); };
  ImageAlign::ComputePoseBatch(pairs, false, &n_meas, &errors, &iters, nullptr, nullptr, s.detected ? nullptr : &detect);
  for (size_t k = 0; k < s.run.size(); k++) {
    FrameStats &st = s.stats[s.run[k]];
    st.align_meas = n_meas[k];
    st.align_iters = iters[k];
    st.align_features = static_cast<int>(pairs[k].first->GetFeatures().size());
  }
}

// stage 2, one host thread per batch (the farm's case): every tracker writes its requests, already in the device layout, straight into
// the pinned staging area of one search batch.  Decides whether the pose stage rides behind the search (chain).
void SDVLBatch::PackRequests(HostStep &s) {
  const int R = s.R();
  int cap = 0;
  for (int k = 0; k < R; k++) cap += static_cast<int>(trk_[s.run[k]]->last_frame_->GetFeatures().size());
  s.sink.ctx = dev_->ctx();
  s.sink.cap = cap;
  // unique per DEVICE, not per SDVLBatch: frames remember the slot they got in a batch by its id, and several SDVLBatches
  // may step on one device
  s.sink.batch_id = ++dev_->search_batch_counter;
  // search -> match selection -> RANSAC + pose refinement as ONE submission (sdvl_search_run_chain): the device replays
  // the second half of SelectPoints itself, so the pose kernels run while this thread does the same replay for its
  // own bookkeeping (features, point statistics) instead of starting after it
  s.chain = s.device_pose && Config::MaxRansacPoints() <= 8;
  for (int k = 0; k < R && s.chain; k++)
    if (trk_[s.run[k]]->feature_align_.MaxMatches() > FeatureAlign::kMaxDevicePoseObs) s.chain = false;
  if (s.chain) {
    if (scratch_points_.size() < 3 * static_cast<size_t>(cap)) scratch_points_.resize(3 * static_cast<size_t>(cap));
    s.sink.points = scratch_points_.data();
  }
  dev_->Check(sdvl_search_begin(s.sink.ctx, cap, &s.sink.reqs), "sdvl_search_begin");
  s.begin.assign(R + 1, 0);
  for (int k = 0; k < R; k++) {
    SDVL &t = *trk_[s.run[k]];
    s.begin[k] = static_cast<size_t>(s.sink.count);
    t.feature_align_.PrepareReprojectPacked(t.current_frame_, t.last_frame_, false, &s.sink);
  }
  s.begin[R] = static_cast<size_t>(s.sink.count);
  s.packed = true;
  if (s.sink.count == 0) s.chain = false;
}

// stage 2, the chain's extra inputs: per tracker the candidates in SelectPoints' order, the draws SelectInliers would make, the start pose
void SDVLBatch::PackChain(HostStep &s) {
  const int R = s.R(), max_its = Config::MaxRansacIts();
  s.chain_frames.resize(R);
  chain_cand_req_.clear();
  chain_cand_first_.clear();
  chain_rand_.clear();
  for (int k = 0; k < R; k++) {
    SDVL &t = *trk_[s.run[k]];
    sdvl_chain_frame &cf = s.chain_frames[k];
    cf.cand_begin = static_cast<int32_t>(chain_cand_req_.size());
    t.feature_align_.EmitChainCandidates(static_cast<int>(s.begin[k]), &chain_cand_req_, &chain_cand_first_);
    cf.cand_end = static_cast<int32_t>(chain_cand_req_.size());
    cf.max_matches = t.feature_align_.MaxMatches();
    cf.rand_begin = static_cast<int32_t>(chain_rand_.size());
    t.feature_align_.PeekRand(max_its, &chain_rand_);
    t.current_frame_->GetPose().ToArray(cf.pose);
    s.chain_obs_begin[k] = k == 0 ? 0 : s.chain_obs_begin[k - 1] + s.chain_frames[k - 1].max_matches;
  }
}

// stage 2 with several host threads: every tracker fills a vector of its own, then all go into scratch_reqs_
void SDVLBatch::CollectRequests(HostStep &s) {
  vector<vector<sdvl_search_req>> per(s.run.size());
  ParallelFor(s.R(), [&](int k) {
    SDVL &t = *trk_[s.run[k]];
    t.feature_align_.PrepareReproject(t.current_frame_, t.last_frame_, false, &per[k]);
  });
  Concatenate(per, &scratch_reqs_, &s.begin);
}

// stage 2: FeatureAlign::Reproject, sdvl.cc:193 — all candidates of all trackers in one launch
void SDVLBatch::LaunchSearch(HostStep &s) {
  const int R = s.R();
  s.Stage(ST_SEARCH);
  if (s.packed) {
    s.res.resize(std::max(1, s.sink.count));
    const sdvl_camera cam = trk_[s.run[0]]->camera_->abi();
    const sdvl_search_params sp = SearchParams();
    if (s.chain) {
      const sdvl_pose_params pp = FeatureAlign::PoseParams(*trk_[s.run[0]]->camera_);
      dev_->Check(sdvl_search_run_chain(s.sink.ctx, s.sink.count, &cam, &sp, s.res.data(), R, s.chain_frames.data(),
                                        static_cast<int>(chain_cand_req_.size()), chain_cand_req_.data(), chain_cand_first_.data(),
                                        scratch_points_.data(), static_cast<int>(chain_rand_.size()), chain_rand_.data(), &pp),
                  "sdvl_search_run_chain");
    } else {
      dev_->Check(sdvl_search_run(s.sink.ctx, s.sink.count, &cam, &sp, s.res.data()), "sdvl_search_run");
    }
  } else if (R > 0) {
    Matcher::SearchPoints(dev_, scratch_reqs_, *trk_[s.run[0]]->camera_, &s.res);
  }
}

// stage 3: replay of SelectPoints, sdvl.cc:193, and the pose jobs of the trackers whose pose the device computes
void SDVLBatch::ReplaySelect(HostStep &s) {
  const int R = s.R();
  s.Stage(ST_FINISH);
  s.pb.resize(threads_ <= 1 ? 0 : R);
  FeatureAlign::PoseBatch &all = scratch_pose_;
  all.jobs.clear(); all.obs.clear(); all.rand_idx.clear(); all.nits.clear();
  s.job_of.assign(R, -1);
  s.on_device.assign(R, 0);
  ParallelFor(R, [&](int k) {
    const int i = s.run[k];
    SDVL &t = *trk_[i];
    FrameStats &st = s.stats[i];
    st.search_requests = static_cast<int>(s.begin[k + 1] - s.begin[k]);
    for (size_t q = s.begin[k]; q < s.begin[k + 1]; q++) st.lk_iters += s.res[q].lk_its;
    t.feature_align_.FinishSelect(t.current_frame_, s.res.data() + s.begin[k], !s.chain);
    t.matches_ = t.feature_align_.GetMatches();
    t.attempts_ = t.feature_align_.GetAttempts();
    if (s.chain) {
      s.job_of[k] = k;  // its pose job is already running
    } else if (s.device_pose) {
      if (threads_ <= 1) {  // sequential: straight into the shared batch
        const int job = static_cast<int>(all.jobs.size());
        s.on_device[k] = t.feature_align_.EmitPoseJob(t.current_frame_, &all) ? 1 : 0;
        if (s.on_device[k]) s.job_of[k] = job;
      } else {
        s.on_device[k] = t.feature_align_.EmitPoseJob(t.current_frame_, &s.pb[k]) ? 1 : 0;
      }
    }
  });
}

// stage 3b: RANSAC + pose refinement (feature_align.cc:73-82,152-243), one launch pair for every tracker — or the wait for the chain's
void SDVLBatch::LaunchPose(HostStep &s) {
  const int R = s.R();
  s.Stage(ST_POSE);
  FeatureAlign::PoseBatch &all = scratch_pose_;
  if (threads_ > 1)
    for (int k = 0; k < R; k++)
      if (s.on_device[k]) {
        s.job_of[k] = static_cast<int>(all.jobs.size());
        all.Append(s.pb[k]);
      }
  if (s.chain) {
    int obs_total = 0;
    for (int k = 0; k < R; k++) obs_total += s.chain_frames[k].max_matches;
    s.pres.resize(R);
    s.lists.resize(obs_total + 1);
    vector<int32_t> n_obs(R);
    dev_->Check(sdvl_search_chain_end(dev_->ctx(), R, s.pres.data(), n_obs.data(), s.lists.data()), "sdvl_search_chain_end");
    for (int k = 0; k < R; k++)
      if (n_obs[k] != trk_[s.run[k]]->feature_align_.FoundCount())
        throw std::runtime_error("SDVLBatch: the device's match selection disagrees with the host replay (" + std::to_string(n_obs[k]) + " vs " +
                                 std::to_string(trk_[s.run[k]]->feature_align_.FoundCount()) + " matches)");
  } else if (!all.jobs.empty()) {
    s.pres.resize(all.jobs.size());
    s.lists.resize(all.obs.size() + 1);
    const sdvl_pose_params pp = FeatureAlign::PoseParams(*trk_[s.run[0]]->camera_);
    dev_->Check(sdvl_pose_from_matches(dev_->ctx(), static_cast<int>(all.jobs.size()), all.jobs.data(), static_cast<int>(all.obs.size()),
                                       all.obs.data(), static_cast<int>(all.rand_idx.size()), all.rand_idx.data(),
                                       static_cast<int>(all.nits.size()), all.nits.data(), &pp, s.pres.data(), s.lists.data()),
                "sdvl_pose_from_matches");
  }
}

// The poses reach the frames (or the host computes them); motion model, tracking quality, keyframe decision — and what the decisions set
// off, sdvl.cc:101-121: feature lists of the points, keyframe graph, retiring the previous frames.
void SDVLBatch::CommitAndSave(HostStep &s) {
  const FeatureAlign::PoseBatch &all = scratch_pose_;
  ParallelFor(s.R(), [&](int k) {
    const int i = s.run[k];
    SDVL &t = *trk_[i];
    FrameStats &st = s.stats[i];
    if (s.job_of[k] >= 0) {
      t.feature_align_.CommitPose(t.current_frame_, s.pres[s.job_of[k]],
                                  s.lists.data() + (s.chain ? s.chain_obs_begin[k] : all.jobs[s.job_of[k]].obs_begin));
    } else {
      t.feature_align_.SelectInliers(t.current_frame_);
      t.feature_align_.OptimizePose(t.current_frame_);
    }
    st.inliers = t.feature_align_.GetInliers();
    st.outliers = t.feature_align_.GetOutliers();
    t.GetMotionModel();
    s.decision[i] = static_cast<char>(t.TrackingDecision());
  });
  // The keyframes are known: the FilterCorners round trip of the fresh ones is queued now and collected in the epilogue, the bookkeeping
  // below runs meanwhile.  Only with one host thread per batch, where that bookkeeping is serial and long enough to hide the round trip;
  // with several the epilogue queues it.
  if (threads_ <= 1) CollectKeyframes(s, true);
  ParallelFor(s.R(), [&](int k) {
    const int i = s.run[k];
    SDVL &t = *trk_[i];
    if (s.decision[i] == 0) return;
    if (s.decision[i] == 2) {
      t.LinkFeatures();
      t.SaveKeyframe(s.stats[i]);
    } else {
      t.map_->AddFrame(t.current_frame_);
    }
    t.last_frame_ = t.current_frame_;
  });
}

// the host-driven form, stage by stage: every request assembled here, results replayed here
void SDVLBatch::HandleFramesGeneric(const vector<Image> &imgs, FrameStats *stats) {
  const int B = static_cast<int>(trk_.size());
  HostStep s(imgs, stats, B);
  for (SDVL *t : trk_) t->track_.valid = false;  // this step changes last_frame's features behind the tables' back
  // ---- stage 0: Frame construction, sdvl.cc:59: the pyramids now, detection behind the image alignment (AlignImages)
  Frame::CreateBatch(trk_[0]->camera_, &trk_[0]->orb_detector_, imgs, false, Config::NumFeatures(), &s.frames, &pfor_);
  for (int i = 0; i < B && !s.detected; i++)
    if (trk_[i]->state_ == SDVL::STATE_RUNNING && trk_[i]->lost_frames_ >= 3) {  // Relocalize searches the new frame in the prelude
      Frame::DetectBatch(s.frames, Config::NumFeatures());
      s.detected = true;
    }
  s.Stage(ST_PRELUDE);
  for (int i = 0; i < B; i++) {
    const FrameStart start = BeginFrame(i, s.frames[i], stats[i]);
    stats[i].host_path = 1;
    if (start == kFirstFrame && trk_[i]->two_frame_init_) s.init.push_back(i);
    if (start == kFirstFrame || (start == kLost && !RelocalizeOnHost(*trk_[i], stats[i]))) continue;
    trk_[i]->SetMotionModel();
    s.run.push_back(i);
  }
  if (!s.init.empty()) InitializeTrackers(s);
  AlignImages(s);
  // ---- stage 2: the search requests, in one of three forms
  s.Stage(ST_PREPARE);
  scratch_reqs_.clear();  // (keeps its capacity from step to step)
  s.chain_obs_begin.assign(s.run.size() + 1, 0);
  if (threads_ <= 1 && !s.run.empty()) {
    PackRequests(s);
    if (s.chain) PackChain(s);
  } else {
    CollectRequests(s);
  }
  LaunchSearch(s);
  ReplaySelect(s);
  LaunchPose(s);
  CommitAndSave(s);
  s.clk.reset();
  EpilogueAndMapper(s);
}

// --------------------------------------------------------------------------------- SDVLBatch: what follows the decisions
// stage 4, the mapper stand-in for the step's keyframes (sequential mode, main.cc:148-149): the second half of their FilterCorners round
// trip, the seeding from the scene plane, and the seeds' rows behind the tables that stayed on the device
void SDVLBatch::FinishKeyframes(Step &s) {
  if (s.kfs.empty()) return;
  Frame::FilterCornersEnd(s.kfs, &pfor_ref_);
  vector<char> appended(s.kfs.size(), 0);
  ParallelFor(static_cast<int>(s.kfs.size()), [&](int k) {
    SDVL &t = *trk_[s.kf_owner[k]];
    PlaneMap *pm = dynamic_cast<PlaneMap *>(t.map_);
    if (pm) pm->SeedFromFiltered(s.kfs[k]);  // other Map implementations run their own mapper on AddKeyframe
    t.pending_kf_ = nullptr;
    if (t.track_.append_pending) {
      t.track_.append_pending = false;
      if (t.track_.valid && AppendSeeds(t, s.kfs[k])) appended[k] = 1;
      else t.track_.valid = false;  // something the rows cannot express: the table is rebuilt from the objects
    }
  });
  vector<int> up;  // the new rows of all keyframes of the step in ONE submission
  for (size_t k = 0; k < s.kfs.size(); k++)
    if (appended[k]) up.push_back(s.kf_owner[k]);
  GatherRows(up, true);
  if (!up.empty())
    dev_->Check(sdvl_track_append(dev_->ctx(), track_, static_cast<int>(up.size()), tr_up_trk_.data(), tr_up_buf_.data(), tr_up_np_.data(), tr_up_points_.data(),
                                  tr_up_nf_.data(), tr_up_feats_.data()), "sdvl_track_append");
}

// what follows the tracking decisions in both forms of a step: the keyframes' FilterCorners round trip + seeding, the
// per-tracker epilogue, and SDVL::Mapping() of sequential mode
void SDVLBatch::EpilogueAndMapper(Step &s) {
  s.Stage(ST_MAPPING);
  if (!s.filter_begun) {  // no keyframe was known early, or the form left the round trip to this thread: counts, then its first half
    FetchCornerCounts(s.frames, s.stats);
    CollectKeyframes(s, false);
  }
  FinishKeyframes(s);
  s.Stage(ST_EPILOGUE);
  ParallelFor(static_cast<int>(trk_.size()), [&](int i) {
    SDVL &t = *trk_[i];
    FrameStats &st = s.stats[i];
    st.quality = static_cast<int>(t.tracking_quality_);
    st.matches = t.matches_;
    st.attempts = t.attempts_;
    t.current_frame_->GetPose().ToArray(st.pose);
    t.stats_ = st;
    t.current_frame_ = nullptr;
    t.map_->EmptyTrash();  // sdvl.cc:127
  });
  s.Stage(ST_MAPPER);
  RunMappers();
  s.clk.reset();
}

// stage 5: SDVL::Mapping() of sequential mode (main.cc:148-149) for the trackers that own a real mapper: the phases of
// Map::UpdateMap run in lock step, every phase's SearchPoint requests of ALL trackers in one K7 launch
void SDVLBatch::RunMappers() {
  vector<MapperMap *> mm;
  {
    StageClock begin_clk(ST_MAP_BEGIN);
    for (SDVL *t : trk_) {
      MapperMap *m = dynamic_cast<MapperMap *>(t->map_);
      if (m && !m->IsThreaded() && m->BeginUpdate()) mm.push_back(m);  // a started mapper thread does its own UpdateMap
    }
  }
  const int M = static_cast<int>(mm.size());
  if (M == 0) return;
  vector<vector<sdvl_search_req>> per(M);
  vector<sdvl_search_res> res;
  vector<size_t> begin(M + 1, 0);
  // UpdateCandidates with the depth filter on the device: one filter state per request, outcomes beside the search results;
  // the rows of the points the trackers follow are patched in the same submission (same context, same stream)
  const bool dev_filter = MapperMap::DeviceFilter();
  vector<vector<sdvl_depth_state>> per_st(M);
  vector<sdvl_depth_state> states;
  vector<sdvl_depth_out> fout;
  const sdvl_depth_params fparams = mm[0]->FilterParams();
  auto launch = [&](bool filter = false) {  // search everything the maps emitted, leave the offsets in `begin`
    // the requests go from the maps' lists straight into the context's pinned batch (device layout, frames by slot)
    Concatenate(per, nullptr, &begin);
    const size_t total = begin[M];
    states.clear();
    res.resize(std::max<size_t>(total, 1));   // every record is written by the call below (no clearing pass over MBs)
    fout.resize(std::max<size_t>(filter ? total : 0, 1));
    if (total == 0) return;
    sdvl_ctx *ctx = dev_->ctx();
    sdvl_search_req_packed *packed = nullptr;
    dev_->Check(sdvl_search_begin(ctx, static_cast<int>(total), &packed), "sdvl_search_begin");
    size_t o = 0;
    for (int k = 0; k < M; k++) {
      for (const sdvl_search_req &r : per[k]) {
        sdvl_search_req_packed &d = packed[o++];
        d.cur = sdvl_search_slot(ctx, r.cur, r.cur_pose);
        d.ref = sdvl_search_slot(ctx, r.ref, r.ref_pose);
        if (d.cur < 0 || d.ref < 0) dev_->Check(d.cur < 0 ? d.cur : d.ref, "sdvl_search_slot");
        d.level = r.level; d.fixed = r.fixed;
        d.px[0] = r.px[0]; d.px[1] = r.px[1];
        d.bearing[0] = r.bearing[0]; d.bearing[1] = r.bearing[1]; d.bearing[2] = r.bearing[2];
        d.idepth = r.idepth; d.idepth_std = r.idepth_std;
        d.px0[0] = r.px0[0]; d.px0[1] = r.px0[1];
        std::memcpy(d.desc, r.desc, 32);
      }
      per[k].clear();
      if (filter) {
        states.insert(states.end(), per_st[k].begin(), per_st[k].end());
        per_st[k].clear();
      }
    }
    const sdvl_camera c = trk_[0]->camera_->abi();
    const sdvl_search_params sp = SearchParams();
    if (filter) {
      if (states.size() != total) throw std::runtime_error("mapper: one filter state per candidate request");
      dev_->Check(sdvl_search_run_filter(ctx, static_cast<int>(total), &c, &sp, states.data(), &fparams, track_, res.data(), fout.data()),
                  "sdvl_search_run_filter");
    } else {
      dev_->Check(sdvl_search_run(ctx, static_cast<int>(total), &c, &sp, res.data()), "sdvl_search_run");
    }
  };
  std::unique_ptr<StageClock> sub(new StageClock(ST_MAP_CANDIDATES));
  for (;;) {  // UpdateCandidates, one occurrence pass at a time
    vector<char> more(M, 0);
    {
      StageClock c(ST_MAP_EMIT);
      ParallelFor(M, [&](int k) { more[k] = mm[k]->EmitCandidates(&per[k], dev_filter ? &per_st[k] : nullptr) ? 1 : 0; });
    }
    if (std::find(more.begin(), more.end(), 1) == more.end()) break;
    {
      StageClock c(ST_MAP_SEARCH);
      launch(dev_filter);
    }
    StageClock c(ST_MAP_APPLY);
    ParallelFor(M, [&](int k) { if (more[k]) mm[k]->ApplyCandidates(res.data() + begin[k], dev_filter ? fout.data() + begin[k] : nullptr); });
  }
  vector<int> kf_idx;
  for (int k = 0; k < M; k++)
    if (mm[k]->IsKeyframeUpdate()) kf_idx.push_back(k);
  const int K = static_cast<int>(kf_idx.size());
  sub.reset(new StageClock(ST_MAP_CONNECTIONS));
  if (K > 0) {
    ParallelFor(K, [&](int q) {
      MapperMap *m = mm[kf_idx[q]];
      m->CheckConnections();
      m->EmitConnectionsPoints(&per[kf_idx[q]]);
    });
    launch();
    vector<char> need(K, 0);
    ParallelFor(K, [&](int q) {
      MapperMap *m = mm[kf_idx[q]];
      m->ApplyConnectionsPoints(res.data() + begin[kf_idx[q]]);
      need[q] = m->PrepareInitCandidates() ? 1 : 0;
    });
    sub.reset(new StageClock(ST_MAP_INIT));
    vector<shared_ptr<Frame>> to_filter;
    for (int q = 0; q < K; q++)
      if (need[q]) to_filter.push_back(mm[kf_idx[q]]->CurrentFrame());
    if (!to_filter.empty()) {
      Frame::FilterCornersBatch(to_filter);
      ParallelFor(K, [&](int q) { if (need[q]) mm[kf_idx[q]]->EmitInitCandidates(&per[kf_idx[q]]); });
      launch();
      ParallelFor(K, [&](int q) { if (need[q]) mm[kf_idx[q]]->ApplyInitCandidates(res.data() + begin[kf_idx[q]]); });
    }
  }
  sub.reset(new StageClock(ST_MAP_FINISH));
  ParallelFor(M, [&](int k) { mm[k]->FinishUpdate(); });
  // local bundle adjustment (map.cc:130-137): the windows of all the step's mappers in ONE sdvl_bundle_adjust call
  bool any_bundle = false;
  for (int k = 0; k < M; k++) any_bundle = any_bundle || mm[k]->BundleAdjustmentOn();
  if (!any_bundle) return;
  sub.reset(new StageClock(ST_MAP_BUNDLE));
  vector<BundleProblem> windows(M);
  vector<char> has(M, 0);
  ParallelFor(M, [&](int k) { has[k] = mm[k]->PrepareBundle(&windows[k]) ? 1 : 0; });
  vector<BundleProblem *> problems;
  vector<int> whose;
  for (int k = 0; k < M; k++)
    if (has[k]) {
      problems.push_back(&windows[k]);
      whose.push_back(k);
    }
  if (problems.empty()) return;
  vector<sdvl_bundle_result> results;
  vector<vector<Frame *>> moved;
  Bundle::Solve(dev_, *trk_[0]->camera_, problems, &results, &moved);
  for (size_t j = 0; j < problems.size(); j++) mm[whose[j]]->FinishBundle(windows[whose[j]], results[j], moved[j]);
}

}  // namespace sdvl
