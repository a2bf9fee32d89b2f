// batch_host_step.cc — SDVLBatch: the host-driven step (HandleFramesGeneric and its stages), the path for what the device-resident
// tables cannot express and the form the tests compare the tabled step with.  Its reusable request / pose batches are
// SDVLBatch::HostScratch; no other file names them.
#include "batch_internal.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace sdvl {

using std::shared_ptr;
using std::vector;

// ------------------------------------------------------------------------------------------ SDVLBatch: the host-driven step
// what the stages of the host-driven form hand to each other on top of Step; index k = position in `run`
struct SDVLBatch::HostStep : SDVLBatch::Step {
  HostStep(const vector<Image> &i, FrameStats *st, int B) : Step(i, st, B), device_pose(DevicePose()) {}
  const bool device_pose;
  // the search requests: in the pinned staging area of one search batch (packed), with the pose stage behind them in the same submission
  // (chain), or in host_scratch_.reqs; those of run[k] are [begin[k], begin[k + 1])
  bool packed = false, chain = false;
  FeatureAlign::PackedSink sink;
  vector<size_t> begin;
  vector<sdvl_chain_frame> chain_frames;
  vector<int> chain_obs_begin;
  vector<sdvl_search_res> res;
  // the pose jobs: per tracker with several host threads, else straight into host_scratch_.pose; job_of[k] = its job there or -1 (host pose)
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
    if (host_scratch_.points.size() < 3 * static_cast<size_t>(cap)) host_scratch_.points.resize(3 * static_cast<size_t>(cap));
    s.sink.points = host_scratch_.points.data();
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
  HostScratch &hs = host_scratch_;
  const int R = s.R(), max_its = Config::MaxRansacIts();
  s.chain_frames.resize(R);
  hs.cand_req.clear();
  hs.cand_first.clear();
  hs.rand.clear();
  for (int k = 0; k < R; k++) {
    SDVL &t = *trk_[s.run[k]];
    sdvl_chain_frame &cf = s.chain_frames[k];
    cf.cand_begin = static_cast<int32_t>(hs.cand_req.size());
    t.feature_align_.EmitChainCandidates(static_cast<int>(s.begin[k]), &hs.cand_req, &hs.cand_first);
    cf.cand_end = static_cast<int32_t>(hs.cand_req.size());
    cf.max_matches = t.feature_align_.MaxMatches();
    cf.rand_begin = static_cast<int32_t>(hs.rand.size());
    t.feature_align_.PeekRand(max_its, &hs.rand);
    t.current_frame_->GetPose().ToArray(cf.pose);
    s.chain_obs_begin[k] = k == 0 ? 0 : s.chain_obs_begin[k - 1] + s.chain_frames[k - 1].max_matches;
  }
}

// stage 2 with several host threads: every tracker fills a vector of its own, then all go into host_scratch_.reqs
void SDVLBatch::CollectRequests(HostStep &s) {
  vector<vector<sdvl_search_req>> per(s.run.size());
  ParallelFor(s.R(), [&](int k) {
    SDVL &t = *trk_[s.run[k]];
    t.feature_align_.PrepareReproject(t.current_frame_, t.last_frame_, false, &per[k]);
  });
  Concatenate(per, &host_scratch_.reqs, &s.begin);
}

// stage 2: FeatureAlign::Reproject, sdvl.cc:193 — all candidates of all trackers in one launch
void SDVLBatch::LaunchSearch(HostStep &s) {
  const HostScratch &hs = host_scratch_;
  const int R = s.R();
  s.Stage(ST_SEARCH);
  if (s.packed) {
    s.res.resize(std::max(1, s.sink.count));
    const sdvl_camera cam = trk_[s.run[0]]->camera_->abi();
    const sdvl_search_params sp = SearchParams();
    if (s.chain) {
      const sdvl_pose_params pp = FeatureAlign::PoseParams(*trk_[s.run[0]]->camera_);
      dev_->Check(sdvl_search_run_chain(s.sink.ctx, s.sink.count, &cam, &sp, s.res.data(), R, s.chain_frames.data(),
                                        static_cast<int>(hs.cand_req.size()), hs.cand_req.data(), hs.cand_first.data(),
                                        hs.points.data(), static_cast<int>(hs.rand.size()), hs.rand.data(), &pp),
                  "sdvl_search_run_chain");
    } else {
      dev_->Check(sdvl_search_run(s.sink.ctx, s.sink.count, &cam, &sp, s.res.data()), "sdvl_search_run");
    }
  } else if (R > 0) {
    Matcher::SearchPoints(dev_, hs.reqs, *trk_[s.run[0]]->camera_, &s.res);
  }
}

// stage 3: replay of SelectPoints, sdvl.cc:193, and the pose jobs of the trackers whose pose the device computes
void SDVLBatch::ReplaySelect(HostStep &s) {
  const int R = s.R();
  s.Stage(ST_FINISH);
  s.pb.resize(threads_ <= 1 ? 0 : R);
  FeatureAlign::PoseBatch &all = host_scratch_.pose;
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
  FeatureAlign::PoseBatch &all = host_scratch_.pose;
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
  const FeatureAlign::PoseBatch &all = host_scratch_.pose;
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
  host_scratch_.reqs.clear();  // (keeps its capacity from step to step)
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

}  // namespace sdvl
