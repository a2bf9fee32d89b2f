// batch.cc — SDVLBatch, the batch driver (B trackers per submission): the worker pool and the process-wide switches; the pieces every
// form of a step shares (BeginFrame, InitializeTrackers, DetectOnSideStream, FetchCornerCounts, CollectKeyframes); HandleFrames; what
// follows the decisions (FinishKeyframes, EpilogueAndMapper, RunMappers).  The other jobs have files of their own: the tracking tables
// (batch_tables.cc), relocalisation inside the tabled step (batch_reloc.cc), the step on the tables (batch_tracked.cc) and the
// host-driven step (batch_host_step.cc).  Reference line numbers are cited at each function; device work goes through the C-ABI
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

const DepthImage *SDVLBatch::DepthOf(int i) const {
  if (!step_depths_ || step_depths_->empty() || (*step_depths_)[i].empty()) return nullptr;
  return &(*step_depths_)[i];
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
      if (staged) (void)sdvl_depth_stage_end(b->dev_->ctx());
    }
  } depth_scope{this, !depths.empty()};
  step_depths_ = &depths;
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
// Depth cameras: the filtered corners of the step's keyframes whose tracker seeds from depth (SDVL::SetDepthSeeding) are looked up in
// their frames' depth images by ONE sdvl_depth_seed call.  (*z)[k] / (*status)[k]: keyframe k's results, null for a keyframe that is not
// seeded from depth.  A keyframe that came without a depth image seeds nothing and is counted.  A first frame becomes the first keyframe
// here if at least SDVL.min_init_corners of its corners have a depth; otherwise it is not kept (its entry of s.kfs becomes null).
void SDVLBatch::SeedKeyframesFromDepth(Step &s, vector<const double *> *z, vector<const uint8_t *> *status) {
  const size_t K = s.kfs.size();
  z->assign(K, nullptr);
  status->assign(K, nullptr);
  bool any = false;
  for (size_t k = 0; k < K; k++) any = any || trk_[s.kf_owner[k]]->depth_seeding_;
  if (!any) return;
  // (a stereo tracker's second image is the pair's right image, SDVL::SetStereoSeeding: the same jobs with sdvl_stereo_depth as the producer)
  vector<sdvl_depth_job> jobs;
  vector<sdvl_stereo_job> pairs;
  vector<size_t> whose;
  vector<int32_t> xyl;
  const sdvl_depth_seed_params *rule = nullptr;
  const sdvl_stereo_params *stereo = nullptr;
  for (size_t k = 0; k < K; k++) {
    SDVL &t = *trk_[s.kf_owner[k]];
    if (!t.depth_seeding_) continue;
    const DepthImage *d = DepthOf(s.kf_owner[k]);
    if (!d) continue;  // (counted below)
    if (t.stereo_seeding_) {
      if (rule || (stereo && std::memcmp(stereo, &t.stereo_rule_, sizeof(*stereo)) != 0))
        throw std::runtime_error("SDVLBatch: the trackers of a batch share the stereo baseline and rule");
      if (d->format != DEPTH_RIGHT8) throw std::runtime_error("SDVLBatch: a tracker that seeds from a stereo pair takes a right image (DEPTH_RIGHT8), not a depth image");
      stereo = &t.stereo_rule_;
    } else {
      if (stereo || (rule && std::memcmp(rule, &t.depth_rule_, sizeof(*rule)) != 0))
        throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth seeding rule");
      rule = &t.depth_rule_;
    }
    const int begin = static_cast<int>(xyl.size() / 3), n = s.kfs[k]->NumFiltered();
    for (int c = 0; c < n; c++) {
      const Vector3i corner = s.kfs[k]->FilteredCorner(c);
      xyl.insert(xyl.end(), {corner(0), corner(1), corner(2)});
    }
    jobs.push_back(sdvl_depth_job{d->data, d->on_device ? 1 : 0, d->step, d->format, 0, d->scale, begin, begin + n});
    pairs.push_back(sdvl_stereo_job{s.kfs[k]->device(), d->data, d->on_device ? 1 : 0, d->step, begin, begin + n});
    whose.push_back(k);
  }
  const int n_corners = static_cast<int>(xyl.size() / 3);
  depth_z_.assign(std::max(n_corners, 1), 0.0);
  depth_status_.assign(std::max(n_corners, 1), 0);
  vector<int32_t> ok(std::max<size_t>(jobs.size(), 1), 0);
  if (!jobs.empty()) {
    const Camera &camera = *trk_[0]->camera_;
    const sdvl_camera cam = camera.abi();
    const sdvl_distortion dist = camera.distortion();
    if (stereo) {
      sdvl_stereo_params sp = *stereo;
      sp.dist = camera.HasDistortion() ? &dist : nullptr;  // (refused: rectified pairs only)
      stereo_disparity_.assign(n_corners, 0.0);
      dev_->Check(sdvl_stereo_depth(dev_->ctx(), static_cast<int>(pairs.size()), pairs.data(), n_corners, xyl.data(), &cam, &sp, depth_z_.data(),
                                    stereo_disparity_.data(), depth_status_.data(), ok.data()),
                  "sdvl_stereo_depth");
    } else {
      dev_->Check(sdvl_depth_seed(dev_->ctx(), static_cast<int>(jobs.size()), jobs.data(), s.kfs[whose[0]]->GetWidth(), s.kfs[whose[0]]->GetHeight(), n_corners,
                                  xyl.data(), &cam, camera.HasDistortion() ? &dist : nullptr, rule, depth_z_.data(), depth_status_.data(), ok.data()),
                  "sdvl_depth_seed");
    }
  }
  for (size_t j = 0; j < jobs.size(); j++) {
    (*z)[whose[j]] = depth_z_.data() + jobs[j].c_begin;
    (*status)[whose[j]] = depth_status_.data() + jobs[j].c_begin;
  }
  size_t j = 0;
  for (size_t k = 0; k < K; k++) {
    SDVL &t = *trk_[s.kf_owner[k]];
    if (!t.depth_seeding_) continue;
    const bool looked_up = j < whose.size() && whose[j] == k;
    if (!looked_up)
      if (PlaneMap *pm = dynamic_cast<PlaneMap *>(t.map_)) pm->CountNoDepth();
    if (t.first_frame_waiting_) {
      if (looked_up && ok[j] >= Config::MinInitCorners()) {
        t.CommitFirstFrame(s.stats[s.kf_owner[k]]);
      } else {  // too few corners with a depth: the frame is not kept, the next one starts over
        t.first_frame_waiting_ = false;
        t.init_failed_ = true;
        t.pending_kf_ = nullptr;
        s.kfs[k] = nullptr;
      }
    }
    if (looked_up) j++;
  }
}

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

// Depth cameras inside the mapper: the filtered corners of all the step's new keyframes whose mapper measures, looked up in their frames'
// depth images by ONE sdvl_depth_seed call (as SeedKeyframesFromDepth does for the keyframes the driver seeds) and handed to the mappers
void SDVLBatch::MeasureKeyframeCorners(const vector<MapperMap *> &mm, const vector<int> &mm_trk, const vector<int> &kf_idx, const vector<char> &need,
                                       const vector<const DepthImage *> &depth_of) {
  vector<sdvl_depth_job> jobs;
  vector<int> whose;
  vector<int32_t> xyl;
  const sdvl_depth_seed_params *rule = nullptr;
  for (size_t q = 0; q < kf_idx.size(); q++) {
    const int k = kf_idx[q];
    if (!need[q] || !mm[k]->DepthMapping()) continue;
    const DepthImage *d = depth_of[k];
    if (!d) {
      mm[k]->SetCornerDepths(nullptr, nullptr);
      continue;
    }
    const sdvl_depth_seed_params *r = &trk_[mm_trk[k]]->depth_rule_;
    if (rule && std::memcmp(rule, r, sizeof(*rule)) != 0) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth seeding rule");
    rule = r;
    const shared_ptr<Frame> &kf = mm[k]->CurrentFrame();
    const int first = static_cast<int>(xyl.size() / 3), n = kf->NumFiltered();
    for (int c = 0; c < n; c++) {
      const Vector3i corner = kf->FilteredCorner(c);
      xyl.insert(xyl.end(), {corner(0), corner(1), corner(2)});
    }
    jobs.push_back(sdvl_depth_job{d->data, d->on_device ? 1 : 0, d->step, d->format, 0, d->scale, first, first + n});
    whose.push_back(k);
  }
  if (jobs.empty()) return;
  const int n_corners = static_cast<int>(xyl.size() / 3);
  depth_z_.assign(std::max(n_corners, 1), 0.0);
  depth_status_.assign(std::max(n_corners, 1), 0);
  vector<int32_t> ok(jobs.size(), 0);
  const Camera &camera = *trk_[0]->camera_;
  const sdvl_camera cam = camera.abi();
  const sdvl_distortion dist = camera.distortion();
  const shared_ptr<Frame> &kf0 = mm[whose[0]]->CurrentFrame();
  dev_->Check(sdvl_depth_seed(dev_->ctx(), static_cast<int>(jobs.size()), jobs.data(), kf0->GetWidth(), kf0->GetHeight(), n_corners, xyl.data(), &cam,
                              camera.HasDistortion() ? &dist : nullptr, rule, depth_z_.data(), depth_status_.data(), ok.data()),
              "sdvl_depth_seed");
  for (size_t j = 0; j < jobs.size(); j++) mm[whose[j]]->SetCornerDepths(depth_z_.data() + jobs[j].c_begin, depth_status_.data() + jobs[j].c_begin);
}

// Depth edges in bundle adjustment (SDVL::SetDepthBundle): the features the step's new keyframes hold when their mapper takes them up —
// the tracked matches, at their found pixel and level — are looked up in their frames' depth images by ONE sdvl_depth_lookup call, inside
// the step's sdvl_depth_stage_begin / _end bracket like the sdvl_depth_seed calls beside it.  A keyframe that is not the step's own frame
// (or came without an image) is not looked up: its image is gone.
void SDVLBatch::LookupKeyframeFeatures(const vector<MapperMap *> &mm, const vector<int> &mm_trk, const vector<int> &kf_idx) {
  vector<sdvl_depth_job> jobs;
  vector<int> whose;
  vector<double> px2;
  vector<int32_t> level;
  const sdvl_depth_seed_params *rule = nullptr;
  int width = 0, height = 0;
  for (int k : kf_idx) {
    if (!mm[k]->DepthBundleOn() || mm[k]->CurrentFrame().get() != trk_[mm_trk[k]]->step_frame_) continue;
    const DepthImage *d = DepthOf(mm_trk[k]);
    if (!d) continue;
    const sdvl_depth_seed_params *r = &trk_[mm_trk[k]]->depth_rule_;
    if (rule && std::memcmp(rule, r, sizeof(*rule)) != 0) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth seeding rule");
    rule = r;
    const int first = static_cast<int>(level.size());
    const int n = mm[k]->EmitDepthLookups(&px2, &level);
    if (n == 0) continue;
    width = mm[k]->CurrentFrame()->GetWidth();
    height = mm[k]->CurrentFrame()->GetHeight();
    jobs.push_back(sdvl_depth_job{d->data, d->on_device ? 1 : 0, d->step, d->format, 0, d->scale, first, first + n});
    whose.push_back(k);
  }
  if (jobs.empty()) return;
  const int n = static_cast<int>(level.size());
  depth_z_.assign(n, 0.0);
  depth_status_.assign(n, 0);
  vector<int32_t> ok(jobs.size(), 0);
  const Camera &camera = *trk_[0]->camera_;
  const sdvl_camera cam = camera.abi();
  const sdvl_distortion dist = camera.distortion();
  dev_->Check(sdvl_depth_lookup(dev_->ctx(), static_cast<int>(jobs.size()), jobs.data(), width, height, n, px2.data(), level.data(), &cam,
                                camera.HasDistortion() ? &dist : nullptr, rule, depth_z_.data(), depth_status_.data(), ok.data()),
              "sdvl_depth_lookup");
  for (size_t j = 0; j < jobs.size(); j++) mm[whose[j]]->ApplyDepthLookups(depth_z_.data() + jobs[j].c_begin, depth_status_.data() + jobs[j].c_begin);
}

// stage 5: SDVL::Mapping() of sequential mode (main.cc:148-149) for the trackers that own a real mapper: the phases of
// Map::UpdateMap run in lock step, every phase's SearchPoint requests of ALL trackers in one K7 launch
void SDVLBatch::RunMappers() {
  vector<MapperMap *> mm;
  vector<int> mm_trk;  // whose mapper mm[k] is
  {
    StageClock begin_clk(ST_MAP_BEGIN);
    for (size_t i = 0; i < trk_.size(); i++) {
      MapperMap *m = AsMapperMap(trk_[i]->map_);
      if (m && !m->IsThreaded() && m->BeginUpdate()) {  // a started mapper thread does its own UpdateMap
        mm.push_back(m);
        mm_trk.push_back(static_cast<int>(i));
      }
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
  // Depth cameras (SDVL::SetDepthMapping): when a mapper of the step has the switch on, the candidate passes go through the measured
  // filter — still one launch for all trackers.  depth_of[k]: the depth image of the step's frame, for a mapper with the switch on whose
  // update works on that very frame; the requests of every other mapper are in no job and take the triangulated rule.
  vector<const DepthImage *> depth_of(M, nullptr);
  const MapperMap *measuring = nullptr;
  for (int k = 0; k < M; k++) {
    if (!mm[k]->DepthMapping()) continue;
    if (!dev_filter) throw std::runtime_error("mapper: depth mapping (SDVL::SetDepthMapping) needs the depth filter on the device");
    const sdvl_depth_measure_params a = mm[k]->DepthMeasureParams(trk_[mm_trk[k]]->depth_rule_);
    if (measuring) {
      const sdvl_depth_measure_params b = measuring->DepthMeasureParams(trk_[mm_trk[k]]->depth_rule_);
      if (a.noise_abs != b.noise_abs || a.noise_quad != b.noise_quad) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth noise parameters");
    }
    measuring = mm[k];
    if (mm[k]->CurrentFrame().get() == trk_[mm_trk[k]]->step_frame_) depth_of[k] = DepthOf(mm_trk[k]);
  }
  vector<uint8_t> depth_status;  // per candidate request, with `measuring`
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
    if (filter && measuring) {
      if (states.size() != total) throw std::runtime_error("mapper: one filter state per candidate request");
      vector<sdvl_depth_job> jobs;
      const sdvl_depth_seed_params *rule = nullptr;
      int width = 0, height = 0;
      for (int k = 0; k < M; k++) {
        const DepthImage *d = depth_of[k];
        if (!d || begin[k] == begin[k + 1]) continue;
        const sdvl_depth_seed_params *r = &trk_[mm_trk[k]]->depth_rule_;
        if (rule && std::memcmp(rule, r, sizeof(*rule)) != 0) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth seeding rule");
        rule = r;
        width = mm[k]->CurrentFrame()->GetWidth();
        height = mm[k]->CurrentFrame()->GetHeight();
        jobs.push_back(sdvl_depth_job{d->data, d->on_device ? 1 : 0, d->step, d->format, 0, d->scale, static_cast<int>(begin[k]), static_cast<int>(begin[k + 1])});
      }
      if (jobs.empty()) { width = 1; height = 1; }  // (no request has an image: nothing is looked up)
      const sdvl_depth_measure_params mp = measuring->DepthMeasureParams(rule ? *rule : sdvl_depth_seed_params{0.0, 0.0, 0.0, 0, 0});
      const Camera &camera = *trk_[0]->camera_;
      const sdvl_distortion dist = camera.distortion();
      depth_status.resize(total);
      dev_->Check(sdvl_search_run_filter_measured(ctx, static_cast<int>(total), &c, &sp, states.data(), &fparams, tables_.set, static_cast<int>(jobs.size()),
                                                  jobs.data(), width, height, camera.HasDistortion() ? &dist : nullptr, &mp, res.data(), fout.data(),
                                                  depth_status.data()),
                  "sdvl_search_run_filter_measured");
    } else if (filter) {
      if (states.size() != total) throw std::runtime_error("mapper: one filter state per candidate request");
      dev_->Check(sdvl_search_run_filter(ctx, static_cast<int>(total), &c, &sp, states.data(), &fparams, tables_.set, res.data(), fout.data()),
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
    ParallelFor(M, [&](int k) {
      if (more[k]) mm[k]->ApplyCandidates(res.data() + begin[k], dev_filter ? fout.data() + begin[k] : nullptr,
                                          measuring && !depth_status.empty() ? depth_status.data() + begin[k] : nullptr);
    });
  }
  vector<int> kf_idx;
  for (int k = 0; k < M; k++)
    if (mm[k]->IsKeyframeUpdate()) kf_idx.push_back(k);
  const int K = static_cast<int>(kf_idx.size());
  sub.reset(new StageClock(ST_MAP_CONNECTIONS));
  if (K > 0) LookupKeyframeFeatures(mm, mm_trk, kf_idx);  // (returns at once unless a mapper has depth edges on)
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
      if (measuring) MeasureKeyframeCorners(mm, mm_trk, kf_idx, need, depth_of);
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
  double bf = 0.0;  // depth edges: the windows of the mappers that have them on carry depths; the trackers of a batch share bf
  for (int k : whose) {
    if (!mm[k]->DepthBundleOn()) continue;
    if (bf > 0.0 && bf != mm[k]->DepthBundleBf()) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth edges' bf");
    bf = mm[k]->DepthBundleBf();
  }
  Bundle::Solve(dev_, *trk_[0]->camera_, problems, &results, &moved, bf);
  for (size_t j = 0; j < problems.size(); j++) mm[whose[j]]->FinishBundle(windows[whose[j]], results[j], moved[j]);
}

}  // namespace sdvl
