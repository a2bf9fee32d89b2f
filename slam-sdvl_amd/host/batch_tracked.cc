// batch_tracked.cc — SDVLBatch: the step on the device-resident tables (HandleFramesTracked and its stages), the look-ahead, and the
// per-object fallback of one tracker inside such a step (TrackOnHost).  The tables themselves are batch_tables.cc's, the relocalisation
// RelocalizeIntoStep calls is batch_reloc.cc's.
#include "batch_internal.h"

#include <algorithm>
#include <stdexcept>

namespace sdvl {

using std::shared_ptr;
using std::vector;

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
  const int R = s.R(), cells = tables_.cells, max_its = Config::MaxRansacIts();
  tables_.jobs.resize(R);
  tables_.rank.resize(static_cast<size_t>(R) * cells);
  tables_.rand.resize(static_cast<size_t>(R) * max_its);
  ParallelFor(R, [&](int k) {
    SDVL &t = *trk_[s.run[k]];
    sdvl_track_job &jb = tables_.jobs[k];
    jb.tracker = s.run[k];
    jb.feat_buf = t.track_.feat_buf;
    jb.last = t.last_frame_->device();
    jb.cur = t.current_frame_->device();
    const SE3 T = t.current_frame_->GetPose() * t.last_frame_->GetPose().Inverse();  // image_align.cc:66
    T.ToArray(jb.T);
    t.last_frame_->GetPose().ToArray(jb.last_pose);
    jb.frame_id = t.current_frame_->GetID();
    jb.max_matches = t.feature_align_.MaxMatches();
    t.feature_align_.ShuffleCellRanks(tables_.rank.data() + static_cast<size_t>(k) * cells);
    t.feature_align_.PeekRand(max_its, tables_.rand.data() + static_cast<size_t>(k) * max_its);
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
  dev_->Check(sdvl_track_align(dev_->ctx(), tables_.set, R, tables_.jobs.data(), tables_.rank.data(), tables_.rand.data(), &cam, &prm), "sdvl_track_align");
  if (!s.detected) {
    DetectOnSideStream(s.frames, fork);  // (no fork: FAST + selection run behind the alignment)
    s.detected = true;
  }
  s.Stage(ST_SEARCH);
  dev_->Check(sdvl_track_search(dev_->ctx(), tables_.set), "sdvl_track_search");
  QueueLookAhead(s);
  tables_.res.resize(R);
  dev_->Check(sdvl_track_collect(dev_->ctx(), tables_.set, R, tables_.res.data()), "sdvl_track_collect");
}

// the step's results: pose, counters, the rand() stream, deletions, motion model, tracking quality, keyframe decision
void SDVLBatch::ReplayTracked(Step &s) {
  const int R = s.R();
  s.Stage(ST_FINISH);
  for (int k = 0; k < R; k++)
    if (tables_.res[k].status != 0) throw std::runtime_error("sdvl_track: a table capacity was exceeded on the device");
  ParallelFor(R, [&](int k) {
    const int i = s.run[k];
    SDVL &t = *trk_[i];
    FrameStats &st = s.stats[i];
    const sdvl_track_result &r = tables_.res[k];
    SDVL::TrackState &ts = t.track_;
    st.align_meas = r.align_meas;
    st.align_iters = r.align_iters;
    st.align_features = r.n_features;
    st.search_requests = r.n_requests;
    st.lk_iters = r.lk_iters;
    st.n_corners = r.n_corners;
    t.current_frame_->SetPose(SE3::FromArray(r.pose));
    t.current_frame_->SetRegistered();  // the step wrote (view, final pose) into the registry
    t.current_frame_->SetFlatFeatures(sdvl_track_features(tables_.set, k), r.matches, ts.points);
    t.current_frame_->SetSceneDepthHint(r.scene_depth);
    const sdvl_track_point_stat *ps = sdvl_track_stats(tables_.set, k);
    ts.stats.assign(ps, ps + ts.points->size());
    ts.stats_dirty = true;
    if (AsMapperMap(t.map_)) SyncStats(t);  // the mapper's depth filter reads and resets the failure counts
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
  for (size_t k = 0; k < s.run.size(); k++) r_matches[s.run[k]] = tables_.res[k].matches;
  ParallelFor(static_cast<int>(act.size()), [&](int a) {
    const int i = act[a];
    SDVL &t = *trk_[i];
    if (s.decision[i] == 0) return;  // tracking lost: last_frame and its table stay
    if (s.decision[i] == 2) {
      // Plane-map trackers: the keyframe's matched features STAY flat records and its table stays the one the step has just left on
      // the device — the points the map seeds in its empty cells are appended to both sides after the seeding (FinishKeyframes ->
      // AppendSeeds -> sdvl_track_append).  The objects appear the first time somebody asks (Frame::GetFeatures()).
      const bool plane = !AsMapperMap(t.map_);
      const size_t rows = t.track_.points ? t.track_.points->size() : static_cast<size_t>(tables_.cap);
      const bool room = static_cast<int>(rows) + tables_.cells <= tables_.cap && r_matches[i] + tables_.cells <= tables_.cap;
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

}  // namespace sdvl
