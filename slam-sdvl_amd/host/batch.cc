// batch.cc — SDVLBatch, the batch driver (B trackers per submission): the worker pool and the process-wide switches; the pieces every
// form of a step shares (BeginFrame, InitializeTrackers, DetectOnSideStream, FetchCornerCounts, CollectKeyframes); HandleFrames; what
// follows the decisions (FinishKeyframes, EpilogueAndMapper).  The other jobs have files of their own: the tracking tables
// (batch_tables.cc), relocalisation inside the tabled step (batch_reloc.cc), the step on the tables (batch_tracked.cc), the
// host-driven step (batch_host_step.cc), the calls that read a frame's depth or right image (batch_depth.cc) and the sequential
// mappers' stage (batch_mapper.cc).  Reference line numbers are cited at each function; device work goes through the C-ABI
// (include/sdvl_hip.h) only.
#include "batch_internal.h"
#include "homography_init.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <thread>

namespace sdvl {

using std::shared_ptr;
using std::vector;

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

SDVLBatch::SDVLBatch(Device *dev, const vector<SDVL *> &trackers, int host_threads)
    : dev_(dev), trk_(trackers), threads_(host_threads), reloc_store_{dev} {
  for (size_t i = 0; i < trk_.size(); i++) trk_[i]->track_.slot = static_cast<int>(i);
  const auto pfor = [this](int n, const std::function<void(int)> &fn) { ParallelFor(n, fn); };
  pfor_ = pfor;
  pfor_ref_ = pfor;
  // A lone camera (a batch of up to four) waits for chains of 0.2 ms: its context polls without sleeping for the first 500 us of a wait (a
  // sleeping poll wakes ~15 us late).  Larger batches keep the sleeping polls: their host threads need the CPU, and a farm waits ~9 ms.
  const int spin_us = trk_.size() <= 4 ? 500 : 0;
  if (dev_ && dev_->ctx()) (void)sdvl_ctx_set_wait_spin(dev_->ctx(), spin_us);
}
SDVLBatch::~SDVLBatch() {  // (the relocalisation store goes with its member, behind this)
  if (tables_.set) {
    Device::SetCurrent(dev_);
    sdvl_track_destroy(dev_->ctx(), tables_.set);
  }
  if (d_rights_) (void)sdvl_device_free(dev_->ctx(), d_rights_);
}

// the calling thread's pool: made at its first ParallelFor, made again when a batch asks for another size, never joined at thread exit
static thread_local Pool *g_pool = nullptr;
static thread_local int g_pool_threads = 0;

void SDVLBatch::ParallelFor(int n, const std::function<void(int)> &fn) {
  if (threads_ <= 1 || n <= 1) {
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  if (g_pool && g_pool_threads != threads_) {
    delete g_pool;
    g_pool = nullptr;
  }
  g_pool_threads = threads_;
  if (!g_pool) g_pool = new Pool(threads_ - 1);
  g_pool->For(n, fn);
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

// ----------------------------------------------------------------------------- SDVLBatch: pieces every form of a step shares
// The common head of a tracker's step, sdvl.cc:59-73: the new frame, and which of three states the tracker is in.  The first frame is
// saved here; what a lost and a running tracker do next is the form's business.
SDVLBatch::FrameStart SDVLBatch::BeginFrame(int i, const shared_ptr<Frame> &frame, FrameStats &st) {
  SDVL &t = *trk_[i];
  st = FrameStats();
  t.current_frame_ = frame;
  t.step_frame_ = frame.get();
  t.current_frame_->SetID(t.frame_counter_++);
  if (t.state_ != SDVL::STATE_RUNNING) {
    if (t.depth_seeding_) {  // the frame becomes the first keyframe in FinishKeyframes, if enough of its corners have a depth
      t.init_failed_ = false;
      if (DepthOf(i)) {
        t.PrepareFirstFrame();
      } else {  // no depth image: the frame is not kept, the next one starts over
        if (PlaneMap *pm = dynamic_cast<PlaneMap *>(t.map_)) pm->CountNoDepth();
        t.init_failed_ = true;
      }
    } else if (!t.two_frame_init_) {
      t.SaveFirstFrame(st);  // otherwise InitializeTrackers, once every tracker's frame is known
    }
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
    const bool fresh = s.decision[i] == 2 && !AsMapperMap(trk_[i]->map_);
    if (trk_[i]->pending_kf_) { s.kfs.push_back(trk_[i]->pending_kf_); s.kf_owner.push_back(static_cast<int>(i)); }
    else if (fresh) { s.kfs.push_back(trk_[i]->current_frame_); s.kf_owner.push_back(static_cast<int>(i)); }
  }
  if (s.kfs.empty()) return;
  std::unique_ptr<StageClock> nested(s.clk->id != ST_MAPPING ? new StageClock(ST_MAPPING) : nullptr);
  if (fetch_counts) FetchCornerCounts(s.frames, s.stats);
  Frame::FilterCornersBegin(s.kfs);
  s.filter_begun = true;
}

void SDVLBatch::HandleFrames(const vector<Image> &imgs, FrameStats *stats) { HandleFrames(imgs, vector<DepthImage>(), stats); }

// SDVL::HandleFrame (sdvl.cc:55-130) for B trackers
void SDVLBatch::HandleFrames(const vector<Image> &imgs, const vector<DepthImage> &depths, FrameStats *stats) {
  const int B = static_cast<int>(trk_.size());
  if (static_cast<int>(imgs.size()) != B) throw std::runtime_error("SDVLBatch::HandleFrames: one image per tracker");
  if (!depths.empty() && static_cast<int>(depths.size()) != B) throw std::runtime_error("SDVLBatch::HandleFrames: one depth image per tracker, or none");
  for (int i = 0; i < B && !depths.empty(); i++)
    if (!depths[i].empty() && (depths[i].cols != imgs[i].cols || depths[i].rows != imgs[i].rows))
      throw std::runtime_error("SDVLBatch::HandleFrames: a depth image has the size of its camera image");
  struct DepthScope {  // the step's depth images are named for the step alone, however it ends
    SDVLBatch *b;
    bool staged;
    ~DepthScope() {
      b->step_depths_ = nullptr;
      b->rights_rectified_ = false;
      if (staged) (void)sdvl_depth_stage_end(b->dev_->ctx());
    }
  } depth_scope{this, !depths.empty()};
  step_depths_ = &depths;
  rights_rectified_ = false;
  Device::SetCurrent(dev_);
  // a pageable depth image is copied to the device once per step: the keyframes' lookup and the mapper's filter passes share the copy
  if (!depths.empty()) dev_->Check(sdvl_depth_stage_begin(dev_->ctx()), "sdvl_depth_stage_begin");
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
    MapperMap *m = AsMapperMap(t->map_);
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

// --------------------------------------------------------------------------------- SDVLBatch: what follows the decisions
// stage 4, the mapper stand-in for the step's keyframes (sequential mode, main.cc:148-149): the second half of their FilterCorners round
// trip, the seeding from the scene plane or from the frames' depth images, and the seeds' rows behind the tables that stayed on the device
void SDVLBatch::FinishKeyframes(Step &s) {
  if (s.kfs.empty()) return;
  Frame::FilterCornersEnd(s.kfs, &pfor_ref_);
  vector<const double *> depth_z;
  vector<const uint8_t *> depth_status;
  SeedKeyframesFromDepth(s, &depth_z, &depth_status);
  vector<char> appended(s.kfs.size(), 0);
  ParallelFor(static_cast<int>(s.kfs.size()), [&](int k) {
    if (!s.kfs[k]) return;  // a first frame that was not kept
    SDVL &t = *trk_[s.kf_owner[k]];
    PlaneMap *pm = dynamic_cast<PlaneMap *>(t.map_);
    // other Map implementations run their own mapper on AddKeyframe
    if (pm && t.depth_seeding_) {
      if (depth_status[k]) pm->SeedFromDepth(s.kfs[k], depth_z[k], depth_status[k]);  // (without a depth image: no seeds)
    } else if (pm) {
      pm->SeedFromFiltered(s.kfs[k]);
    }
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
    dev_->Check(sdvl_track_append(dev_->ctx(), tables_.set, static_cast<int>(up.size()), tables_.up_trk.data(), tables_.up_buf.data(), tables_.up_np.data(),
                                  tables_.up_points.data(), tables_.up_nf.data(), tables_.up_feats.data()), "sdvl_track_append");
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

}  // namespace sdvl
