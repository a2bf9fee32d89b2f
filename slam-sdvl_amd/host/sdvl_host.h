// sdvl_host.h — host side of the MI355X-native SDVL front-end: the reference's C++ API surface
// (Camera, Feature, Point, Frame, FastDetector, ORBDetector, ImageAlign, Matcher, FeatureAlign, SDVL) with the same
// names, argument meaning and return conventions, implemented on top of the C-ABI in include/sdvl_hip.h.
//
// MI355X-first differences (none visible to a caller that uses the reference signatures):
//   * a Frame's pyramid / corners / descriptors live in HBM; GetPyramid() / GetDescriptors() mirror to the host
//     lazily (the mapper and the UI read them);
//   * every stage has a batched form (Frame::CreateBatch, ImageAlign::ComputePoseBatch, Matcher::SearchPoints,
//     FeatureAlign::PrepareReproject/FinishReproject, SDVLBatch::HandleFrames) so that B independent sequences
//     advance one frame with ONE launch per kernel; the single-object calls are the B = 1 case;
//   * FeatureAlign evaluates Matcher::SearchPoint for ALL grid candidates in one launch and then replays the
//     reference's sequential cell-order / first-hit / max_matches logic over the results (SearchPoint is a pure
//     function of its arguments, so the outcome is identical to the one-call-at-a-time loop).
// Error convention: the reference returns bool/int and prints to cerr; so does this layer.  A failing device call
// is fatal (std::runtime_error carrying sdvl_last_error) — there is no CPU fallback.
// Round 4: the header is in three parts — frontend_deps.h (Camera, Point, Map: the reference tree's own classes), frontend.h (the hot
// path's classes) and, below, what only the standalone build needs: the map stand-ins and SDVL.  The batch driver, SDVLBatch, has a
// header of its own, batch.h, which this one includes at its end.
#ifndef SDVL_HOST_H_
#define SDVL_HOST_H_

#include "frontend.h"
#include "bundle.h"

namespace sdvl {

// Map stand-in for synthetic scenes: seeds one FIXED point per FilterCorners() corner of a keyframe, depth from a
// known scene plane n.X = d (stands in for homography_init + depth filter).
class PlaneMap : public Map {
 public:
  PlaneMap(const Vector3d &n, double d) : n_(n), d_(d) {}
  void InitCandidates(const std::shared_ptr<Frame> &kf) override;
  void SeedFromFiltered(const std::shared_ptr<Frame> &kf);  // after Frame::FilterCorners()
  void SetPlane(const Vector3d &n, double d) { n_ = n; d_ = d; }
  // Depth cameras: the sibling of SeedFromFiltered for a keyframe whose filtered corners have been looked up in a registered depth image
  // (sdvl_depth_seed: z[k] metres along the optical axis and status[k] of filtered corner k).  Every corner with status OK gets the feature
  // and the descriptor SeedFromFiltered gives it and a FIXED point at s = z / v_z along its bearing v — the same variance (0.05 / s)^2 and
  // the same bookkeeping, so the tracking tables take its rows unchanged; every other corner gets no point.  The plane is not read.
  void SeedFromDepth(const std::shared_ptr<Frame> &kf, const double *z, const uint8_t *status);
  // what depth seeding did so far: keyframes seeded, points seeded, the corners by status (sdvl_depth_seed's codes, [0] = OK), and the
  // keyframes (or first frames) of a depth-seeding tracker that arrived without a depth image
  struct DepthStats { long keyframes = 0, seeds = 0, by_status[5] = {0, 0, 0, 0, 0}, no_depth = 0; };
  const DepthStats &GetDepthStats() const { return depth_stats_; }
  void CountNoDepth() { depth_stats_.no_depth++; }
  // the live points seeded from depth, oldest first: position, the frame id of their keyframe, their corner (level coordinates, level)
  struct SeededPoint { double x, y, z; int keyframe_id, u, v, level; };
  std::vector<SeededPoint> GetSeededPoints() const;
  // Round 5: the stub honours SDVL.max_keyframes like the reference's map (map.cc:190-205,692-706: once the list is full, the
  // keyframe furthest from the new one goes to the trash) — and, being the owner of the points it seeded there, deletes the points
  // whose FIRST observation lies in the culled keyframe with it (the reference keeps a culled keyframe's image alive for as long as
  // any point names it; here the HBM frame goes back to the pool, so whole sequences run in bounded memory).  The oracle's plane
  // map does the same (oracle/ref_tracker.h); with the reference's cfg values (max_keyframes 1000) S-A never gets there.
  void LimitKeyframes(const std::shared_ptr<Frame> &frame) override;
  void EmptyTrash() override;

 protected:
  struct DepthSeedRec { std::weak_ptr<Point> point; int keyframe_id, u, v, level; };
  std::vector<DepthSeedRec> depth_seeds_;  // SeedFromDepth drops the records of points that are gone
  bool store_depths_ = false;              // MapperMap::SetDepthBundle: a seeded corner's feature keeps its z (Feature::SetDepth)
  DepthBundleStats depth_bundle_stats_;

 private:
  Vector3d n_;
  double d_;
  std::vector<std::shared_ptr<Frame>> culled_;
  DepthStats depth_stats_;
};

// map.h:44-139 — the reference's mapper in SEQUENTIAL mode (main.cc:148-149: SDVL::Mapping() = Map::UpdateMap() after every
// frame).  The first keyframe is bootstrapped from the scene plane unless the tracker takes the two-frame initialisation
// (SDVL::SetTwoFrameInit, homography_init.cc); every later
// keyframe goes through UpdateCandidates / CheckConnections / AddConnectionsPoints / InitCandidates, ordinary frames
// through UpdateCandidates / CheckRedundantKeyframes.  Local bundle adjustment (map.cc:130-137) runs behind them when SetBundleAdjustment(true).
// Every SearchPoint the mapper would issue one at a time is emitted as a request instead (Emit*), evaluated for MANY
// trackers in one K7 launch, and the reference's sequential logic is replayed over the results (Apply*) — the same
// speculate-then-replay scheme FeatureAlign uses (SearchPoint is a pure function of its arguments).
class MapperMap : public PlaneMap {
 public:
  MapperMap(const Vector3d &n, double d, Camera *camera) : PlaneMap(n, d), camera_(camera) {}
  void AddKeyframe(const std::shared_ptr<Frame> &frame, bool search = true) override;  // map.cc:143-158
  void AddFrame(const std::shared_ptr<Frame> &frame) override { frame_queue_.push_back(frame); }
  void LimitKeyframes(const std::shared_ptr<Frame> &frame) override;                   // map.cc:190-205
  void SetRelocalizing(bool v) override { relocalizing_ = v; }
  void EmptyTrash() override;
  void InitCandidates(const std::shared_ptr<Frame> &) override {}  // the bootstrap keyframe is seeded by the driver

  // ---- Map::UpdateMap (map.cc:75-141) cut into phases; a driver calls them in this order for all its trackers
  bool BeginUpdate();                                            // pops the next frame; false = nothing to do
  // UpdateCandidates, one pass; false = no more passes.  states / fout: the depth filter runs on the device behind the search
  // (sdvl_search_points_filter) and Apply only books its outcomes; without them Apply does the arithmetic itself
  bool EmitCandidates(std::vector<sdvl_search_req> *reqs, std::vector<sdvl_depth_state> *states = nullptr);
  // status (with fout): the depth lookup's byte per request, from sdvl_search_run_filter_measured; counted into DepthMapStats
  void ApplyCandidates(const sdvl_search_res *res, const sdvl_depth_out *fout = nullptr, const uint8_t *status = nullptr);
  static bool DeviceFilter();             // env SDVL_HOST_DEPTH_FILTER=1 turns it off
  static void SetDeviceFilter(bool on);
  sdvl_depth_params FilterParams() const;

  bool IsKeyframeUpdate() const { return cur_ && cur_->IsKeyframe(); }
  void CheckConnections();                                       // map.cc:500-558
  void EmitConnectionsPoints(std::vector<sdvl_search_req> *reqs);  // AddConnectionsPoints, map.cc:560-617
  void ApplyConnectionsPoints(const sdvl_search_res *res);
  bool PrepareInitCandidates();                                  // map.cc:262-283; true = the keyframe needs FilterCorners
  const std::shared_ptr<Frame> &CurrentFrame() const { return cur_; }
  void EmitInitCandidates(std::vector<sdvl_search_req> *reqs);   // after Frame::FilterCorners of CurrentFrame()
  void ApplyInitCandidates(const sdvl_search_res *res);
  // ---- depth cameras inside the mapper (an addition; SDVL::SetDepthMapping).  The driver's side of it: UpdateCandidates goes through
  // sdvl_search_run_filter_measured with the depth image of the step's frame, and between Frame::FilterCorners and EmitInitCandidates
  // the filtered corners of the new keyframe are looked up in that image (sdvl_depth_seed) and handed over here: z[c] / status[c] of
  // filtered corner c, null: no image.  A corner with status OK is MEASURED, at the range z / bearing.z along its bearing:
  //   * its requests say so to the search: idepth = 1 / range, idepth_std = the tau_inverse of the measured filter for that range;
  //   * found in a connected keyframe and not linked to a point there, it becomes a point at the measured range — no triangulation, no
  //     parallax test, the two minimum-depth tests on the range — with both features, fixed at once (map.cc:385-389) and pushed ONCE;
  //   * neither linked nor found in any connected keyframe, it becomes a fixed point with its one observation on the new keyframe, made
  //     as PlaneMap::SeedFromDepth makes the bootstrap keyframe's, behind the loop over the connected keyframes, in corner order.
  // Unmeasured corners go the reference's way.  Needs the depth filter on the device and the sequential mapper.
  void SetDepthMapping(bool on, double noise_abs = 0.0, double noise_quad = 0.0);
  bool DepthMapping() const { return depth_mapping_; }
  sdvl_depth_measure_params DepthMeasureParams(const sdvl_depth_seed_params &rule) const { return sdvl_depth_measure_params{rule, noise_abs_, noise_quad_}; }
  void SetCornerDepths(const double *z, const uint8_t *status);
  // ---- stereo cameras inside the mapper (an addition; SDVL::SetStereoMapping): the same machinery with the other producer.  The
  // second image of the step's frame is the pair's right image; UpdateCandidates goes through sdvl_search_run_filter_stereo (the matcher
  // at the found pixel), the new keyframe's filtered corners through sdvl_stereo_depth, whose z / status SetCornerDepths takes as it takes
  // sdvl_depth_seed's (OK is 0 in both status families).  The depth noise is tau = disparity_sigma z^2 / fb, fb = fx x baseline in
  // pixel x metres; disparity_sigma 0: SDVL_STEREO_DISPARITY_SIGMA (0.25 px, not measured against a real pair).  The counters are
  // DepthMapStats, fallback[] by the matcher's status (NOMATCH, AMBIGUOUS, EDGE, OUTSIDE).  Throws as SetDepthMapping does, and
  // std::invalid_argument for a disparity_sigma that is negative or not finite or an fb that is not positive.
  void SetStereoMapping(bool on, double disparity_sigma, double fb);
  bool StereoMapping() const { return stereo_mapping_; }
  bool Measuring() const { return depth_mapping_ || stereo_mapping_; }
  double DisparitySigma() const { return disparity_sigma_; }  // as given (0: the default)
  // candidate updates that took the measured depth and those that fell back by the lookup's status (HOLE, FEW, EDGE, OUTSIDE); keyframes
  // whose corners were looked up; corners fixed from depth and matched in a connected keyframe, fixed on the new keyframe alone, and
  // measured corners that were linked to an existing point
  struct DepthMapStats { long measured = 0, fallback[4] = {0, 0, 0, 0}, keyframes = 0, fixed_matched = 0, fixed_unmatched = 0, linked = 0; };
  const DepthMapStats &GetDepthMapStats() const { return depth_map_stats_; }
  void FinishUpdate();                                           // CheckRedundantKeyframes + trash for ordinary frames
  // ---- local bundle adjustment, the end of Map::UpdateMap (map.cc:130-137) and Map::BundleAdjustment (map.cc:844-869); off by default.
  // Sequential mode only: throws while the mapper thread runs, and Start() throws while it is on.
  void SetBundleAdjustment(bool on);
  bool BundleAdjustmentOn() const { return bundle_on_; }
  // the window of ba_kf_, if the map has more than `min_keyframes` keyframes and a keyframe is waiting (:131-132; SaveSecondFrame asks
  // without the size test, sdvl.cc:172).  false: nothing to solve — no waiting keyframe, a keyframe without connections (:860-861), no
  // points (bundle.cc:91-92), or more free poses than SDVL_BUNDLE_MAX_FREE (skipped and counted)
  bool PrepareBundle(BundleProblem *out, int min_keyframes = 2);
  // behind Bundle::Solve: books the result; the keyframes that moved leave the device's pose registry, the tracking tables and the
  // relocalisation store are told that they are stale
  void FinishBundle(const BundleProblem &problem, const sdvl_bundle_result &result, const std::vector<Frame *> &moved);
  void BundleAdjustment(int min_keyframes = 2);  // the three for this map alone: one sdvl_bundle_adjust call
  const BundleStats &GetBundleStats() const { return bundle_stats_; }
  // ---- depth edges in the adjustment (an addition; SDVL::SetDepthBundle, off by default).  An observation carries the camera-frame z its
  // frame's depth image measured at it when the feature was made in a step that had the image: the corners a keyframe is seeded from
  // (PlaneMap::SeedFromDepth, the measured corners of InitCandidates) keep sdvl_depth_seed's z, and the features a frame holds when it
  // becomes a keyframe — its tracked matches — are looked up at their found pixel and level (sdvl_depth_lookup, by the driver: the
  // two calls below).  Features added to a keyframe in a later step (AddConnectionsPoints, the partner feature of a new candidate in a
  // connected keyframe) carry none and stay monocular edges.  bf (pixel x metres) turns depth noise into pixels; 0: 1 / noise_quad of
  // SetDepthMapping (0.0015 when that is off or at its default, 666.7 px m): one pixel of the third residual is then one sigma of the
  // quadratic noise term — an order of magnitude nobody has measured against a sensor, like that term.  Throws std::runtime_error
  // without bundle adjustment on and while the mapper thread runs, std::invalid_argument for a negative or non-finite bf.
  void SetDepthBundle(bool on, double bf = 0.0);
  bool DepthBundleOn() const { return depth_bundle_; }
  double DepthBundleBf() const { return depth_bundle_bf_ > 0.0 ? depth_bundle_bf_ : 1.0 / (noise_quad_ != 0.0 ? noise_quad_ : SDVL_DEPTH_NOISE_QUAD); }
  // the features of CurrentFrame() (a keyframe update) that have no depth yet, as level-0 positions and levels, appended to the lists
  int EmitDepthLookups(std::vector<double> *px2, std::vector<int32_t> *level);
  void ApplyDepthLookups(const double *z, const uint8_t *status);  // of the features EmitDepthLookups listed, in its order
  const DepthBundleStats &GetDepthBundleStats() const { return depth_bundle_stats_; }
  // the whole of it for one tracker (one launch per phase)
  void UpdateMap() override;
  // map.cc:49-71: the mapper thread of threaded mode.  It works on a Device of its own (one sdvl_ctx = one HIP stream per
  // host thread, include/sdvl_hip.h) on the tracker's GPU and shares the tracker's frames read-only.
  ~MapperMap() override;
  void Start() override;
  void Stop() override;
  void Run();
  long Updates() const { return updates_; }  // UpdateMap calls that found a frame to work on
  bool IsThreaded() const { return running_; }

  // map.h: Map::AddCandidate — a point of the two-frame initialisation enters the depth filter's list (homography_init.cc:171)
  void AddCandidate(const std::shared_ptr<Point> &p) { candidates_.push_back(p); version_++; }

  struct Stats { int candidates = 0, converged = 0, initialized = 0, linked = 0, connected = 0, keyframes = 0; };
  Stats GetStats() const;
  // The live points the mapper created, x y z fixed each: keyframes oldest first, each keyframe's features in order, each point once;
  // deleted points and points first seen on the bootstrap keyframe (they come from the plane itself) are left out.  Host state: a
  // batch's caller runs SDVLBatch::SyncHostState first.
  struct MapPoint { double x, y, z; bool fixed; };
  std::vector<MapPoint> GetMapPoints() const;

 private:
  void CheckRedundantKeyframes();  // map.cc:619-690
  bool CornerMeasured(int c) const { return static_cast<size_t>(c) < ic_range_.size() && ic_range_[c] > 0.0; }
  double MeasuredTauInverse(double range, double z) const;
  Camera *camera_;
  std::vector<std::shared_ptr<Point>> candidates_;
  std::deque<std::shared_ptr<Frame>> frame_queue_, keyframe_queue_;
  std::vector<std::shared_ptr<Frame>> frame_trash_, retired_;  // retired_: culled keyframes stay alive while features name them
  int num_kfs_ = 0, initial_kf_id_ = 0, last_kf_checked_ = -1;
  bool relocalizing_ = false;
  Stats stats_;
  bool bundle_on_ = false;
  std::shared_ptr<Frame> ba_kf_;  // map.h:125: the keyframe waiting for its bundle adjustment (set in AddKeyframe)
  BundleStats bundle_stats_;
  // state of the update in flight
  std::shared_ptr<Frame> cur_;
  double depth_mean_ = 0.0;
  int pass_ = 0, req_base_ = 0;
  enum CandState { kDeleted, kInvisible, kTooClose, kSearch };
  struct CandWork { size_t index; int req; CandState state; };  // position in candidates_, request (relative) or -1, decision before the search
  std::vector<CandWork> cand_work_;
  std::vector<int> occurrence_;                            // per candidates_ entry: which occurrence of its point it is
  std::vector<std::pair<std::shared_ptr<Point>, int>> acp_work_;  // AddConnectionsPoints: point, request or -1
  std::vector<std::shared_ptr<Frame>> best_kfs_;
  std::vector<int> ic_req_;                                // InitCandidates: request of (kf k, filtered corner c) or -1
  std::vector<std::shared_ptr<Feature>> ic_feature_;
  struct KfScan { double x, y; bool live; };
  std::vector<KfScan> kf_scan_;                            // InitCandidates: a connected keyframe's features as the seed loop scans them
  std::vector<sdvl_search_req> ic_proto_;                  // InitCandidates: the request of filtered corner c without its keyframe
  bool depth_mapping_ = false;
  double noise_abs_ = 0.0, noise_quad_ = 0.0;              // SetDepthMapping: as given (0: sdvl_depth_measure_params' default)
  bool stereo_mapping_ = false;
  double disparity_sigma_ = 0.0;                           // SetStereoMapping: as given (0: SDVL_STEREO_DISPARITY_SIGMA)
  // the noise MeasuredTauInverse applies, RESOLVED: a depth camera's pair with its defaults put in, a stereo rig's exactly 0 and
  // disparity_sigma / fb (a 0 here is a 0, not "take the default")
  double tau_abs_ = SDVL_DEPTH_NOISE_ABS, tau_quad_ = SDVL_DEPTH_NOISE_QUAD;
  std::vector<double> ic_range_;                           // SetCornerDepths: the measured range of filtered corner c, 0: not measured
  std::vector<double> ic_z_;                               // and the sample itself, for Feature::SetDepth
  bool depth_bundle_ = false;
  double depth_bundle_bf_ = 0.0;                           // SetDepthBundle: as given (0: the default)
  std::vector<std::shared_ptr<Feature>> lookup_features_;  // EmitDepthLookups: whose depths ApplyDepthLookups gets
  DepthMapStats depth_map_stats_;
  std::thread thread_;
  std::atomic<bool> running_{false};
  std::atomic<long> updates_{0};
  Device *tracker_device_ = nullptr;  // whose GPU and point-id sequence the mapper thread joins
};

typedef std::pair<std::shared_ptr<Point>, Vector2d> PointInfo;
typedef std::list<PointInfo> GridCell;

class SDVLBatch;
class HomographyInit;

// sdvl.h:36-108.  By default the first frame becomes a keyframe at `first_pose` and the Map seeds its points from a scene plane
// (PlaneMap for synthetic scenes); SetTwoFrameInit(true) takes the reference's two-frame homography bootstrap instead.
class SDVL {
 public:
  enum State { STATE_FIRST_FRAME, STATE_SECOND_FRAME, STATE_RUNNING };
  enum TrackingQuality { TRACKING_GOOD, TRACKING_INSUFFICIENT, TRACKING_BAD };
  // sdvl.h:49: the tracker owns its map (the reference's mapper, MapperMap).  Unless SetTwoFrameInit(true) is called,
  // the first keyframe's points come from a scene plane: z = Config::MapScale() in the first camera's frame (the
  // depth the reference's initialisation normalises the map to) unless SetBootstrapPlane says otherwise.  A Device for the
  // calling thread is created if none is bound yet (GPU 0, or SDVL_GPU).
  explicit SDVL(Camera *camera);
  // additions: a caller-owned map (PlaneMap stub or MapperMap) and first pose — what SDVLBatch's trackers are built with
  SDVL(Camera *camera, Map *map, const SE3 &first_pose = SE3());
  ~SDVL();
  void SetBootstrapPlane(const Vector3d &n, double d);
  // The reference's first-frame / second-frame states (sdvl.cc:132-177, HomographyInit) instead of the plane bootstrap: the first
  // frame's filtered corners are tracked (device KLT) until their median shift reaches SDVL.min_avg_shift, then a homography is
  // fitted (device RANSAC), decomposed and triangulated, and the points enter the map as depth-filter candidates.  Needs the
  // reference's mapper (MapperMap): throws std::runtime_error with any other map.  Not built: Map::TransformInitialMap (the world
  // frame stays the first camera's).  Deviation: an initialisation that fails with empty lists (sdvl.cc:66-69,
  // where the reference stays stuck) makes HandleFrame return false and starts over with the next frame as first frame.
  void SetTwoFrameInit(bool on);
  bool TwoFrameInit() const { return two_frame_init_; }
  // Depth cameras (an addition): every keyframe this tracker's map would seed from the scene plane — each one with the plane map, the
  // bootstrap keyframe with the reference's mapper, which carries on as after the plane bootstrap — is seeded from the registered depth
  // image handed over with its frame instead (HandleFrame(img, depth), SDVLBatch::HandleFrames(imgs, depths, stats)): metric scale, no
  // plane, any scene geometry.  `rule`: sdvl_depth_seed_params, zero fields take the defaults; the trackers of one batch share it.
  // A keyframe that arrives without a depth image seeds nothing and is counted (PlaneMap::GetDepthStats).  A first frame without a depth
  // image, or with fewer OK seeds than SDVL.min_init_corners, is not kept: HandleFrame returns false and the next frame starts over (the
  // deviation SetTwoFrameInit documents).  Throws std::runtime_error together with the two-frame initialisation — the two answer the same
  // question — and with a map that is neither PlaneMap nor MapperMap; std::invalid_argument for a rule sdvl_depth_seed would refuse.
  void SetDepthSeeding(bool on, const sdvl_depth_seed_params &rule = sdvl_depth_seed_params{0.0, 0.0, 0.0, 0, 0});
  bool DepthSeeding() const { return depth_seeding_; }
  // Stereo cameras (an addition): depth seeding's keyframe path with another producer.  The second image handed over with a frame is the
  // pair's rectified RIGHT image (a DepthImage of format DEPTH_RIGHT8: 8-bit gray, the camera image's size and intrinsics, the right camera
  // `baseline` metres along the left camera's x axis); the filtered corners of the step's keyframes are matched in it by ONE
  // sdvl_stereo_depth call, and z / status go where sdvl_depth_seed's go: every keyframe of a plane map, the bootstrap keyframe of the
  // reference's mapper.  `rule`: sdvl_stereo_params, zero fields take the defaults (its baseline and dist are ignored); the trackers of
  // one batch share baseline and rule.  First frames as with SetDepthSeeding: one without a right image, or with fewer OK corners than
  // SDVL.min_init_corners, is not kept.  Throws std::runtime_error together with the two-frame initialisation, with depth seeding from a
  // depth image, with depth mapping or depth edges (both look depths up at found pixels, which a matcher at the corners does not give),
  // on a camera with a lens (rectified pairs only; a calibrated rig goes through SetStereoRectification) and with a map that is neither PlaneMap nor MapperMap; std::invalid_argument for a
  // baseline or a rule sdvl_stereo_depth would refuse.
  void SetStereoSeeding(bool on, double baseline, const sdvl_stereo_params &rule = sdvl_stereo_params{0.0, 0.0, 0.0, 0, 0, 0, 0, nullptr});
  bool StereoSeeding() const { return stereo_seeding_; }
  // Stereo rigs as calibrated (an addition): the tracker's Camera is the RECTIFIED camera of `pair` (RectifiedPair::Plan of the rig; the
  // camera built from pair.camera(), no lens), and HandleFrame(img, right) takes the RAW images of both cameras.  The left one is
  // rectified inside its frame's upload (sdvl_frames_upload_rectified, where a lens takes sdvl_frames_upload_undistorted); the right
  // one into HBM, once per step for all trackers of a batch in ONE sdvl_rectify call, and only in a step that has a consumer for it (a
  // keyframe to seed, stereo mapping).  Everything behind sees a rectified pair; poses are the rectified left camera's (R1 of the
  // pair's left side takes the raw left camera's frame to it).  The trackers of one batch share the pair.  Throws std::runtime_error
  // without stereo seeding, on a camera with a lens of its own, when the camera's intrinsics or size differ from the pair's, when the
  // baseline of SetStereoSeeding differs from the pair's by more than 1e-12 relative, and with the mapper thread started;
  // Start() throws while it is on.  The switch and the pair are kept on the Camera (Camera::rectified_pair): trackers that share a Camera
  // share them.  SetStereoSeeding(false) and SetDepthSeeding(false) turn it off too.
  void SetStereoRectification(const RectifiedPair &pair, bool on = true);
  bool StereoRectification() const { return camera_->rectified_pair() != nullptr; }
  // Depth cameras inside the reference's mapper (an addition, MapperMap::SetDepthMapping): the depth image of every tracked frame feeds
  // the candidates' depth filter, and a new keyframe's corners become fixed points at their measured depth.  noise: the sensor's depth
  // noise tau = noise_abs + noise_quad z^2 (0: 0.001 m and 0.0015 per metre); the trackers of a batch share it.  Needs SetDepthSeeding and
  // the reference's mapper in sequential mode with the depth filter on the device: throws std::runtime_error without depth seeding, with
  // any other map, while the mapper thread runs (and Start() throws while it is on), and with the host depth filter.
  void SetDepthMapping(bool on, double noise_abs = 0.0, double noise_quad = 0.0);
  // Stereo cameras inside the reference's mapper (an addition, MapperMap::SetStereoMapping): the right image of every tracked frame feeds
  // the candidates' depth filter through the matcher at the found pixel (sdvl_search_run_filter_stereo), and a new keyframe's corners
  // become fixed points at the depth sdvl_stereo_depth gives them — what SetDepthMapping does for a depth camera.  Off by default; a
  // frame that comes without a right image is mapped as before.  disparity_sigma: the matcher's disparity noise in pixels, depth noise
  // tau = disparity_sigma z^2 / (fx baseline); 0: 0.25 px, an order of magnitude that nobody has measured against a real pair (on the
  // synthetic `shelf` scene the matcher's median error is 0.04 - 0.07 px); the trackers of a batch share it.  Throws std::runtime_error
  // without stereo seeding, with any map but the reference's mapper, while the mapper thread runs (and Start() throws while it is on)
  // and with the host depth filter; std::invalid_argument for a negative or non-finite disparity_sigma.  While it is on,
  // SetStereoSeeding(false) and SetDepthSeeding(false) throw.
  void SetStereoMapping(bool on, double disparity_sigma = 0.0);
  // Map::BundleAdjustment after every keyframe update of a map with more than two keyframes (map.cc:130-137), on the device
  // (sdvl_bundle_adjust).  Off by default.  Needs the reference's mapper in sequential mode: throws std::runtime_error with any other map
  // and while the mapper thread runs.
  void SetBundleAdjustment(bool on);
  // Depth edges in that adjustment (an addition, MapperMap::SetDepthBundle): the observations that carry a measured depth become
  // EdgeStereoSE3ProjectXYZ edges (sdvl_bundle_adjust_depth), which fixes the scale that a window with one fixed keyframe leaves free.
  // Off by default.  bf: pixel x metres, 0 takes 1 / noise_quad of the depth mapping.  Throws std::runtime_error without depth seeding,
  // without bundle adjustment on, with any other map and while the mapper thread runs; std::invalid_argument for a negative or
  // non-finite bf.  Depth mapping is not required.
  void SetDepthBundle(bool on, double bf = 0.0);
  // sdvl.h:52-54 (the UI's queries)
  void GetCameraTrail(std::vector<std::pair<SE3, bool>> *positions);
  void GetPoints(std::vector<Vector3d> *positions);
  void GetLastFeatures(std::vector<Vector3i> *positions);
  // sdvl.h:58-60: Start / Stop the mapper thread (threaded mode, main.cc:120); Mapping() = one mapper step (sequential mode)
  void Start() { map_->Start(); }
  void Stop() { map_->Stop(); }
  void Mapping();
  bool HandleFrame(const Image &img);
  bool HandleFrame(const Image &img, const DepthImage &depth);  // SetDepthSeeding: the frame's registered depth image; SetStereoSeeding: the pair's right image (empty: none)
  // Round 5, an addition for callers that READ a sequence (main.cc's Video.type 1: images from disk are there before they are needed):
  // name the image the NEXT HandleFrame call will be given (a device image, e.g. what Camera::UndistortImage returns, kept alive and
  // unchanged until that call).  Its pyramid and corner detection are queued behind the coming call's chain and run while the host
  // finishes that call.  Same results; an unused or mismatching look-ahead is dropped.
  void SetNextImage(const Image &next);
  SE3 GetPose() const;
  TrackingQuality GetTrackingQuality() const { return tracking_quality_; }
  bool HasMap() { return state_ == STATE_RUNNING; }
  const FrameStats &LastStats() const { return stats_; }
  Map *GetMap() { return map_; }
  // wall clock per host stage of this tracker's own HandleFrame calls (null before the first call); diagnostic
  const StageTimes *HandleFrameStageTimes() const;

 private:
  friend class SDVLBatch;
  void CalcTrackingQuality(int matches, int attempts);
  // the per-frame logic of HandleFrame (sdvl.cc:55-130) that every form of SDVLBatch's step shares
  void SetMotionModel();
  void GetMotionModel();
  void ResetMotionModel();
  void SaveFirstFrame(FrameStats &st);
  // SaveFirstFrame in two halves for a depth-seeding tracker: the frame takes the first pose and waits for its corners' depth lookup;
  // it becomes the first keyframe once enough of them have a depth (SDVLBatch::FinishKeyframes)
  void PrepareFirstFrame();
  void CommitFirstFrame(FrameStats &st);
  bool depth_seeding_ = false, first_frame_waiting_ = false;
  const Frame *step_frame_ = nullptr;  // the frame of the step in flight (BeginFrame): whose depth image the step's is
  sdvl_depth_seed_params depth_rule_ = {0.0, 0.0, 0.0, 0, 0};
  bool stereo_seeding_ = false;  // depth_seeding_ with sdvl_stereo_depth as the producer (SetStereoSeeding)
  sdvl_stereo_params stereo_rule_ = {0.0, 0.0, 0.0, 0, 0, 0, 0, nullptr};
  bool InitFirstFrame(FrameStats &st);                       // sdvl.cc:132-148 (two-frame initialisation)
  void SecondFrameDone(bool initialised, FrameStats &st);    // sdvl.cc:154-176 behind HomographyInit::InitSecondFrame
  bool two_frame_init_ = false, init_failed_ = false;
  std::unique_ptr<HomographyInit> h_init_;
  int TrackingDecision();
  void StartRelocalizing();
  void Relocalized(const std::shared_ptr<Frame> &kf, FrameStats &st);
  void LinkFeatures();
  void SaveKeyframe(FrameStats &st);
  std::unique_ptr<Device> own_device_;  // SDVL(Camera*) on a thread without a Device
  std::unique_ptr<Map> own_map_;        // SDVL(Camera*): the reference's `Map map_` member
  Camera *camera_;
  Map *map_;
  ORBDetector orb_detector_;
  RandStream rng_;
  State state_ = STATE_FIRST_FRAME;
  std::shared_ptr<Frame> current_frame_, last_frame_, last_kf_, pending_kf_;
  TrackingQuality tracking_quality_ = TRACKING_GOOD;
  Vector6d vel_;
  FeatureAlign feature_align_;
  int lost_frames_ = 0, matches_ = 0, attempts_ = 0;
  int frame_counter_ = 0;
  SE3 first_pose_;
  FrameStats stats_;
  bool relocalize_pending_ = false;
  // Round 5: HandleFrame() steps through a batch of one that LIVES with the tracker, so a lone camera gets the device-resident
  // tracking tables too — a tracked frame is one submission and one wait instead of the host-driven stage-by-stage form
  std::unique_ptr<SDVLBatch> self_batch_;
  std::vector<Image> next_image_;  // SetNextImage: handed to the batch by the HandleFrame call it belongs to
  void SyncSelfBatch();
  // device-resident tracking table of this tracker (SDVLBatch owns the set): valid = the table holds last_frame_'s features
  struct TrackState {
    bool valid = false;
    int feat_buf = 0;
    int slot = 0;                                     // the tracker's index in its batch = which table of the set is its own
    const void *owner = nullptr;                      // the SDVLBatch whose set holds that table (a tracker may be stepped by a farm batch AND through HandleFrame)
    std::shared_ptr<Frame::PointTable> points;        // table index -> Point
    std::vector<sdvl_track_point_stat> stats;         // newest counters of `points`; the Point objects lag behind
    bool stats_dirty = false;
    // rows of a rebuilt table on their way to the device (every tracker fills its own: the rebuilds of a step run in parallel)
    std::vector<sdvl_track_point> up_points;
    std::vector<sdvl_track_feature> up_feats;
    std::vector<Frame *> up_register;                 // keyframes the registry does not know yet
    // round 4: the step made the frame a keyframe and left the table current on the device: the rows of the points the map seeds on
    // it are APPENDED (sdvl_track_append) instead of the table being rebuilt from objects; first_seed = the keyframe's object
    // features before the seeding (what comes behind are the seeds)
    bool append_pending = false;
    size_t first_seed = 0;
  } track_;
  // Relocalize (sdvl.cc:205-238) aligns every new frame against the same keyframes: their feature records live in the batch's
  // sdvl_align_store from the first lost frame until the map changes (Map::Version)
  struct RelocCache {
    const void *owner = nullptr;               // the SDVLBatch whose store holds the records
    unsigned long long version = ~0ull;        // Map::Version() the records were packed at
    unsigned long long epoch = 0;              // the store's epoch (a store that was reset has lost them)
    std::vector<std::shared_ptr<Frame>> kfs;   // newest first, the order Relocalize visits them in
    std::vector<int32_t> begin;                // kfs.size() + 1 record offsets in the store
    std::vector<double> T;                     // 7 per keyframe: start pose * keyframe pose^-1 (image_align.cc:66 with frame2 at the keyframe's pose)
  } reloc_;
};

}  // namespace sdvl

#include "batch.h"  // SDVLBatch, the batch driver SDVL::HandleFrame steps through

#endif  // SDVL_HOST_H_
