// farm.cc — TrackerGroup and TrackerFarm (farm.h): the device side of a group-step, the worker threads and fibers that run them, the
// feeder thread of host-fed runs and the run's timeline.  The bookkeeping they share is FarmSchedule (farm_schedule.h).
#include "farm.h"

#include <malloc.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <time.h>
#include <ucontext.h>

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <stdexcept>
#include <thread>

#include "sampling_profile.h"

namespace sdvl {

// ---- TrackerGroup ----------------------------------------------------------------------------------------------------
TrackerGroup::TrackerGroup(Device *dev, int B, int w, int h, const double *cam4, const double *plane4, const double *first_poses7,
                           int host_threads, bool use_mapper)
    : dev_(dev), w_(w), h_(h) {
  Device::SetCurrent(dev_);
  cam_.reset(new Camera(w, h, cam4[0], cam4[1], cam4[2], cam4[3]));
  std::vector<SDVL *> raw;
  for (int i = 0; i < B; i++) {
    if (use_mapper) maps_.emplace_back(new MapperMap(Vector3d(plane4[0], plane4[1], plane4[2]), plane4[3], cam_.get()));
    else maps_.emplace_back(new PlaneMap(Vector3d(plane4[0], plane4[1], plane4[2]), plane4[3]));
    trackers_.emplace_back(new SDVL(cam_.get(), maps_.back().get(), SE3::FromArray(first_poses7 + 7 * i)));
    raw.push_back(trackers_.back().get());
  }
  batch_.reset(new SDVLBatch(dev_, raw, host_threads));
}

TrackerGroup::~TrackerGroup() {
  Device::SetCurrent(dev_);
  batch_.reset();
  trackers_.clear();
  maps_.clear();
}

std::vector<Image> TrackerGroup::Wrap(Frames where, const void *const *imgs, int stride) const {
  std::vector<Image> v;
  v.reserve(trackers_.size());
  for (size_t i = 0; i < trackers_.size(); i++) {
    v.push_back(where == Frames::kHost ? Image::Wrap(static_cast<const uint8_t *>(imgs[i]), w_, h_, stride)
                                       : Image::WrapDevice(imgs[i], w_, h_, stride, true, where == Frames::kTransient));
    v.back().raw = v.back().raw || raw_input_;
    v.back().format = format_;
  }
  return v;
}

void TrackerGroup::Step(Frames where, const void *const *imgs, int stride, FrameStats *out) {
  for (size_t i = 0; i < trackers_.size(); i++) out[i] = FrameStats();
  batch_->HandleFrames(Wrap(where, imgs, stride), out);
}

void TrackerGroup::Step(Frames where, const void *const *imgs, int stride, const void *const *depths, FrameStats *out) {
  for (size_t i = 0; i < trackers_.size(); i++) out[i] = FrameStats();
  std::vector<DepthImage> d;
  if (depths) {
    const int bps = depth_format_ == DEPTH_RIGHT8 ? 1 : depth_format_ == DEPTH_U16 ? 2 : 4;
    for (size_t i = 0; i < trackers_.size(); i++)
      d.push_back(depths[i] ? DepthImage::Wrap(depths[i], w_, h_, w_ * bps, depth_format_, depth_scale_, where != Frames::kHost) : DepthImage());
  }
  batch_->HandleFrames(Wrap(where, imgs, stride), d, out);
}

void TrackerGroup::SetDepth(bool on, int format, double scale, const sdvl_depth_seed_params &rule) {
  if (format != DEPTH_F32 && format != DEPTH_U16) throw std::invalid_argument("TrackerGroup::SetDepth: unknown depth format " + std::to_string(format));
  if (format == DEPTH_U16 && !(scale > 0.0)) throw std::invalid_argument("TrackerGroup::SetDepth: a 16-bit depth image needs scale > 0 (metres per unit)");
  for (auto &t : trackers_) t->SetDepthSeeding(on, rule);
  depth_format_ = format;
  depth_scale_ = scale;
}

void TrackerGroup::SetStereoMapping(bool on, double disparity_sigma) {
  for (auto &t : trackers_) t->SetStereoMapping(on, disparity_sigma);
}

void TrackerGroup::SetStereo(bool on, double baseline, const sdvl_stereo_params &rule) {
  for (auto &t : trackers_) t->SetStereoSeeding(on, baseline, rule);
  if (on) {
    depth_format_ = DEPTH_RIGHT8;
    depth_scale_ = 1.0;
  } else if (depth_format_ == DEPTH_RIGHT8) {
    depth_format_ = DEPTH_F32;
  }
}

void TrackerGroup::SetStereoRectification(const RectifiedPair &pair, bool on) {
  for (auto &t : trackers_) t->SetStereoRectification(pair, on);
}

void TrackerGroup::SetNextImages(const void *const *dev_imgs, int stride) {
  batch_->SetNextImages(dev_imgs ? Wrap(Frames::kResident, dev_imgs, stride) : std::vector<Image>());
}

void TrackerGroup::SetDistortion(const double *dist5) {
  cam_->SetDistortions(dist5[0], dist5[1], dist5[2], dist5[3], dist5[4]);
  raw_input_ = cam_->HasDistortion();
}

void TrackerGroup::SetColor(int format) {
  if (PixelFormatBytes(format) == 0) throw std::invalid_argument("TrackerGroup::SetColor: unknown pixel format " + std::to_string(format));
  format_ = format;
}

// ---- cooperative group-steps -----------------------------------------------------------------------------------------
// A group-step spends ~40 % of its time blocked on its own stream (alignment, search, pose, filter results).  With
// fibers_per_worker_ > 1 a worker thread runs several group-steps on separate stacks (ucontext); the library's wait hook
// (sdvl_ctx_set_wait_hook) switches to another fiber whenever a step would sleep, and the thread only sleeps — a 25 us
// nanosleep between polls, no spinning: the CPU quota is the scarce resource — when every fiber is waiting for the GPU.
namespace {
// a fiber's stack: 1 MB with an inaccessible page below it, so that an overflow (deep recursion in the mapper or the HIP
// runtime) faults instead of silently overwriting the heap
struct FiberStack {
  static constexpr size_t kBytes = 1 << 20, kGuard = 4096;
  char *base = nullptr;
  FiberStack() {
    void *p = mmap(nullptr, kBytes + kGuard, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_STACK, -1, 0);
    if (p == MAP_FAILED) throw std::bad_alloc();
    base = static_cast<char *>(p);
    mprotect(base, kGuard, PROT_NONE);
  }
  ~FiberStack() { if (base) munmap(base, kBytes + kGuard); }
  FiberStack(const FiberStack &) = delete;
  FiberStack &operator=(const FiberStack &) = delete;
  char *data() const { return base + kGuard; }
  size_t size() const { return kBytes; }
};
}  // namespace

struct TrackerFarm::Fiber {
  ucontext_t ctx;
  FiberStack stack;
  TrackerFarm *farm = nullptr;
  int group = -1;  // -1 = free
  int step = 0;
  bool finished = true, whole_run = false;  // whole_run: the fiber owns its group, all steps back to back
  sdvl_ctx *waiting_on = nullptr;
  // per-thread state of the host layer, saved across switches
  Device *tls_device = nullptr;
  StageTimes *tls_stage = nullptr;
};
struct TrackerFarm::FiberScheduler {
  ucontext_t main;
  Fiber *current = nullptr;
};
thread_local TrackerFarm::FiberScheduler *TrackerFarm::fiber_sched_ = nullptr;

void TrackerFarm::FiberWaitHook(void *, sdvl_ctx *ctx) {
  FiberScheduler *s = fiber_sched_;
  if (!s || !s->current) {  // not on a fiber (plain batch use): sleep like the default wait
    sdvl_ctx_wait_block(ctx);
    return;
  }
  Fiber *f = s->current;
  f->waiting_on = ctx;
  f->tls_device = Device::Current();
  f->tls_stage = StageTimes::Active();
  swapcontext(&f->ctx, &s->main);
  Device::SetCurrent(f->tls_device);
  StageTimes::Active() = f->tls_stage;
  f->waiting_on = nullptr;
}

// A fiber's stack cannot be unwound past this function: everything it calls reports through the schedule (StepGroup catches).
void TrackerFarm::FiberMain(unsigned lo, unsigned hi) {
  Fiber *f = reinterpret_cast<Fiber *>((static_cast<uintptr_t>(hi) << 32) | lo);
  if (f->whole_run) {
    for (int s = 0; s < f->farm->n_steps_ && f->farm->StepAndFinish(f->group, s); s++) {}
  } else {
    f->farm->StepAndFinish(f->group, f->step);
  }
  f->finished = true;
  // returning ends the context: uc_link takes the thread back to the scheduler
}

// ---- TrackerFarm -----------------------------------------------------------------------------------------------------
TrackerFarm::TrackerFarm(int gpu, int G, int Bg, int w, int h, const double *cam4, const double *plane4, const double *first_poses7,
                         int host_threads_per_group, bool use_mapper)
    : gpu_(gpu), G_(G), Bg_(Bg), w_(w), h_(h), ring_(G, nullptr) {
  // G host threads allocate and free small objects all the time while their keyframes keep ~100 KB each for good: with the
  // default settings every per-thread malloc arena grows in 128 KB steps (one mprotect each, all serialised on the process's
  // address-space lock together with the page faults) and gives memory back as eagerly.  Grow in 32 MB steps, never trim.
  mallopt(M_TOP_PAD, 32 << 20);
  mallopt(M_TRIM_THRESHOLD, 1 << 30);
  mallopt(M_MMAP_THRESHOLD, 16 << 20);
  for (int g = 0; g < G; g++) {
    devices_.emplace_back(new Device(gpu));
    groups_.emplace_back(new TrackerGroup(devices_.back().get(), Bg, w, h, cam4, plane4, first_poses7 + static_cast<size_t>(7) * g * Bg,
                                          host_threads_per_group, use_mapper));
  }
}

TrackerFarm::~TrackerFarm() {
  groups_.clear();
  if (feed_) sdvl_feed_destroy(feed_);  // waits for its stream: nothing writes the rings after this
  for (size_t g = 0; g < devices_.size(); g++)
    if (ring_[g]) sdvl_device_free(devices_[g]->ctx(), ring_[g]);
  devices_.clear();
}

void TrackerFarm::Reserve(int frames_per_group) {
  for (auto &d : devices_) d->Reserve(w_, h_, Config::PyramidLevels(), frames_per_group);
}

void TrackerFarm::SetFibers(int n) {
  fibers_per_worker_ = n > 1 ? n : 1;
  for (auto &d : devices_) sdvl_ctx_set_wait_hook(d->ctx(), fibers_per_worker_ > 1 ? FiberWaitHook : nullptr, nullptr);
}

void TrackerFarm::SetHostInput(bool on) {
  host_input_ = on;
  if (!UsesRing()) return;
  // the input rings are allocated here, not inside the first host-fed step (hipMalloc synchronises the device); the feed itself is
  // created by the first host-fed run, which also reports a ring that could not be allocated
  const size_t fb = static_cast<size_t>(w_) * h_;
  for (int g = 0; g < G_; g++)
    if (!ring_[g] && sdvl_device_malloc(devices_[g]->ctx(), static_cast<int64_t>(kRingSlots * fb * Bg_), &ring_[g]) != SDVL_OK) ring_[g] = nullptr;
}

void TrackerFarm::SetColor(int format) {
  for (auto &g : groups_) g->SetColor(format);
  format_ = format;
}

TrackerFarm::FeedStats TrackerFarm::feed_stats() const {
  FeedStats s = stats_;
  s.feed_wait_s = sched_.feed_wait_s();
  s.work_wait_s = sched_.work_wait_s();
  return s;
}

void *TrackerFarm::RingSlot(int g, int s) const {
  return static_cast<uint8_t *>(ring_[g]) + static_cast<size_t>(s % kRingSlots) * Bg_ * w_ * h_;
}

// Step s of group g, on the calling thread or fiber.  No exception leaves it: a failure is a status and its message.
int TrackerFarm::StepGroup(int g, int s, std::string *message) noexcept {
  try {
    const int total = G_ * Bg_;
    const size_t off = static_cast<size_t>(s) * total + static_cast<size_t>(g) * Bg_;
    TrackerGroup &grp = *groups_[g];
    if (UsesRing()) {
      StepGroupOnRing(g, s, out_ + off);
    } else if (host_input_) {
      grp.Step(TrackerGroup::Frames::kHost, frames_ + off, stride_, out_ + off);
    } else {
      // frames resident in HBM: the group knows its next images — their pyramids and detection are queued a step ahead (SDVL_NO_LOOKAHEAD=1: A/B)
      static const bool lookahead = getenv("SDVL_NO_LOOKAHEAD") == nullptr;
      if (lookahead && s + 1 < n_steps_) grp.SetNextImages(frames_ + off + total, stride_);
      grp.Step(TrackerGroup::Frames::kResident, frames_ + off, stride_, out_ + off);
    }
    return 0;
  } catch (const std::exception &e) {
    *message = e.what();
  } catch (...) {
    *message = "unknown exception in a group-step";
  }
  return -1;
}

// the host-fed form: the images of the step are in (or on their way into) the group's ring slot
void TrackerFarm::StepGroupOnRing(int g, int s, FrameStats *out) {
  sdvl_ctx *ctx = devices_[g]->ctx();
  if (!sched_.WaitIssued(g, s)) throw std::runtime_error("the run has failed");  // an echo: the cause is already booked
  const double t_issued = Since();
  const int slot = g * kRingSlots + s % kRingSlots;
  const bool late = sdvl_feed_slot_arrived(feed_, slot) == 0;  // statistics only: this step starts behind a transfer still under way
  // The step is submitted only once its images are in HBM: a stream that waits for a transfer ON THE DEVICE holds a barrier
  // packet in its hardware queue, and the streams that share the queue (4 queues for 16 groups) stall behind it although their
  // own images arrived long ago.
  if (late) {
    const auto tw = std::chrono::steady_clock::now();
    for (;;) {
      const int a = sdvl_feed_slot_arrived(feed_, slot);
      if (a < 0) throw std::runtime_error(std::string("input ring: ") + sdvl_feed_last_error(feed_));
      if (a != 0) break;
      timespec ts{0, 50000};
      nanosleep(&ts, nullptr);
    }
    const double dw = std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    std::lock_guard<std::mutex> lk(stats_m_);
    stats_.late_acquires++;
    stats_.arrive_wait_s += dw;
  }
  const double t_enter = Since();
  if (sdvl_ctx_feed_acquire(ctx, feed_, slot) != SDVL_OK)  // this step's kernels start behind its images
    throw std::runtime_error(std::string("input ring: ") + sdvl_last_error(ctx));
  const size_t fb = static_cast<size_t>(w_) * h_;
  std::vector<const void *> src(Bg_);
  for (int i = 0; i < Bg_; i++) src[i] = static_cast<uint8_t *>(RingSlot(g, s)) + i * fb;
  groups_[g]->Step(TrackerGroup::Frames::kTransient, src.data(), w_, out);
  // the kernels queued up to here (the keyframes' copy out of the slot included) are the slot's last readers
  if (sdvl_ctx_feed_release(ctx, feed_, slot) != SDVL_OK) throw std::runtime_error(std::string("input ring: ") + sdvl_last_error(ctx));
  if (timeline_) {
    StepMark k{g, s, t_enter, t_issued, Since(), late ? 1 : 0, {0}, 0};
    const double *now_t = groups_[g]->batch().stage_times.t;
    for (int i = 0; i < kTimelineStages; i++) k.st[i] = now_t[i] - mark_prev_[g][i];
    mark_prev_[g].assign(now_t, now_t + ST_COUNT);
    for (int i = 0; i < Bg_; i++) k.kf += out[i].keyframe ? 1 : 0;
    step_marks_[g].push_back(k);
  }
}

// one group-step and its bookkeeping; false: it failed, nothing more of this group is to be run
bool TrackerFarm::StepAndFinish(int g, int s) {
  std::string message;
  const int rc = StepGroup(g, s, &message);
  sched_.Finish(g, rc, message);
  return rc == 0;
}

// The feeder: queues the images of (group, step) pairs on the farm's one copy stream, always for the group whose next step is
// the earliest among those with a free ring slot (FarmSchedule::NextFeed).
void TrackerFarm::RunFeeder() {
  const size_t fb = static_cast<size_t>(w_) * h_;
  const int total = G_ * Bg_;
  std::vector<void *> dst(Bg_);
  std::deque<int> in_flight;  // slots whose transfer has been queued and not yet seen complete, oldest first
  constexpr int feed_in_flight = 2;  // at most two transfers queued on the device (one: the link idles between them; more: no gain)
  for (;;) {
    int s = 0;
    const int g = sched_.NextFeed(true, &s);
    if (g < 0) return;
    // At most feed_in_flight transfers are queued on the device at any time.  Every queued transfer is handed to a DMA engine at
    // once and sits there waiting for its predecessor; with a ring's worth of them queued (48) every engine of the GPU holds one,
    // and the small DMA copies of the compute streams (FilterCorners records, 1 MB) wait behind 79-MB transfers for tens of ms.
    while (static_cast<int>(in_flight.size()) >= feed_in_flight) {
      const int a = sdvl_feed_slot_arrived(feed_, in_flight.front());
      if (a < 0) {
        sched_.Fail(std::string("input ring: ") + sdvl_feed_last_error(feed_));
        return;
      }
      if (a == 1) { in_flight.pop_front(); continue; }
      const auto tw = std::chrono::steady_clock::now();
      timespec ts{0, 50000};
      nanosleep(&ts, nullptr);
      stats_.feed_throttle_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    }
    const auto tc = std::chrono::steady_clock::now();
    const double tm0 = Since();
    const int slot = g * kRingSlots + s % kRingSlots;
    for (int i = 0; i < Bg_; i++) dst[i] = static_cast<uint8_t *>(RingSlot(g, s)) + i * fb;
    const size_t o = static_cast<size_t>(s) * total + static_cast<size_t>(g) * Bg_;
    const int rc = sdvl_feed_images(feed_, slot, Bg_, reinterpret_cast<const uint8_t *const *>(frames_ + o), stride_, w_, h_, dst.data());
    stats_.feed_call_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count();
    stats_.feed_calls++;
    in_flight.push_back(slot);
    if (timeline_) feed_marks_.push_back(FeedMark{g, s, tm0, Since()});
    sched_.BookFeed(g, rc == SDVL_OK ? 0 : -1, rc == SDVL_OK ? std::string() : std::string("input ring: ") + sdvl_feed_last_error(feed_));
  }
}

// With one worker per group every worker owns its group for the whole run: the group's host objects stay in that
// thread's caches and allocator arena (measured +8 % over handing group-steps out dynamically).  With fewer workers
// than groups a worker repeatedly takes the idle group that is furthest behind (FarmSchedule::TakeGroup).
void TrackerFarm::RunShare(int worker, int n_workers) {
  if (n_workers == G_) {
    const bool marks_here = timeline_ && !UsesRing();
    for (int s = 0; s < n_steps_ && !sched_.Failed(); s++) {
      std::string message;
      const double tb = marks_here ? Since() : 0.0;
      const int rc = StepGroup(worker, s, &message);
      if (marks_here) step_marks_[worker].push_back(StepMark{worker, s, tb, tb, Since(), 0, {0}, 0});
      sched_.Finish(worker, rc, message);
      if (rc != 0) return;
    }
    return;
  }
  for (;;) {
    int s = 0;
    const int g = sched_.TakeGroup(true, &s);
    if (g < 0) return;
    StepAndFinish(g, s);
  }
}

void TrackerFarm::RunShareFibers(int worker, int n_workers) {
  FiberScheduler sched;
  fiber_sched_ = &sched;
  prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);  // a 25 us nanosleep should cost ~30 us, not 25 + the default 50 us slack
  std::vector<Fiber> fibers(fibers_per_worker_);
  int idle_polls = 0;
  auto start = [&](Fiber &f, int g, int s, bool whole_run) {
    f.farm = this;
    f.group = g;
    f.step = s;
    f.finished = false;
    f.whole_run = whole_run;
    f.waiting_on = nullptr;
    getcontext(&f.ctx);
    f.ctx.uc_stack.ss_sp = f.stack.data();
    f.ctx.uc_stack.ss_size = f.stack.size();
    f.ctx.uc_link = &sched.main;
    const uintptr_t p = reinterpret_cast<uintptr_t>(&f);
    makecontext(&f.ctx, reinterpret_cast<void (*)()>(FiberMain), 2, static_cast<unsigned>(p & 0xFFFFFFFFu), static_cast<unsigned>(p >> 32));
  };
  // as many groups as fibers in the farm: every fiber owns one group for the whole run (same reason as in RunShare)
  const bool owned = n_workers * fibers_per_worker_ == G_;
  if (owned)
    for (int i = 0; i < fibers_per_worker_; i++) start(fibers[i], worker * fibers_per_worker_ + i, 0, true);
  bool no_more = owned;
  for (;;) {
    int active = 0;
    for (Fiber &f : fibers) {  // give every free fiber a group-step
      if (f.group < 0 && !no_more) {
        int s = 0;
        const int g = sched_.TakeGroup(false, &s);
        if (g == FarmSchedule::kNothingLeft) no_more = true;
        if (g >= 0) start(f, g, s, false);
      }
      if (f.group >= 0) active++;
    }
    if (active == 0) {
      if (no_more) break;
      int s = 0;
      const int g = sched_.TakeGroup(true, &s);  // everything left is busy on other workers: wait for one (or for the end)
      if (g < 0) break;
      StepAndFinish(g, s);  // no fiber needed: nothing else to overlap with right now
      continue;
    }
    bool progressed = false;
    for (Fiber &f : fibers) {
      if (f.group < 0) continue;
      if (f.waiting_on && !sdvl_ctx_wait_done(f.waiting_on)) continue;  // its stream is still busy
      sched.current = &f;
      swapcontext(&sched.main, &f.ctx);
      sched.current = nullptr;
      progressed = true;
      if (f.finished) f.group = -1;
    }
    if (!progressed) {  // every fiber waits for the GPU: sleep a poll interval (any of their streams may finish first)
      const struct timespec ts = {0, 25000};
      nanosleep(&ts, nullptr);
      if (++idle_polls % 2048 == 0) {  // ~every 100 ms without progress: a faulted stream never reaches its mark
        for (Fiber &f : fibers)
          if (f.group >= 0 && f.waiting_on && sdvl_ctx_health(f.waiting_on) != SDVL_OK)
            sched_.Fail(std::string("GPU fault while a group-step was waiting: ") + sdvl_last_error(f.waiting_on));
        if (sched_.Failed()) break;  // the fibers' stacks are abandoned: the run is over
      }
    } else {
      idle_polls = 0;
    }
  }
  fiber_sched_ = nullptr;
}

void TrackerFarm::WriteTimeline(const char *path) const {
  FILE *fp = std::fopen(path, "a");
  if (!fp) return;
  std::fprintf(fp, "# run: %d groups x %d steps\n", G_, n_steps_);
  for (const auto &v : step_marks_)
    for (const auto &k : v) {
      std::fprintf(fp, "step %d %d %.6f %.6f %.6f %d kf %d stages", k.g, k.s, k.t_enter, k.t_issued, k.t_end, k.late, k.kf);
      for (int i = 0; i < kTimelineStages; i++) std::fprintf(fp, " %.4f", k.st[i]);
      std::fprintf(fp, "\n");
    }
  for (const auto &k : feed_marks_) std::fprintf(fp, "feed %d %d %.6f %.6f\n", k.g, k.s, k.t0, k.t1);
  std::fclose(fp);
}

// The threads are created per run on purpose: measured on the MI355X hosts, freshly forked threads are spread over idle
// cores by the scheduler, while long-lived workers woken through a condition variable are pulled next to their waker
// and run ~6 % slower (80.0k vs 75.6k tracked frames/s at 120 steps); creating 16 threads costs well under a millisecond.
void TrackerFarm::Run(int n_steps, const void *const *frames, int stride, FrameStats *out, int workers) {
  const int W = workers > 0 ? (workers < G_ ? workers : G_) : G_;
  // one byte per pixel rides the host input: gray, and the Bayer mosaics, which are converted inside the step like any colour frame
  if (host_input_ && PixelFormatBytes(format_) != 1)
    throw std::runtime_error("TrackerFarm::Run: colour frames need frames resident in HBM; the host input and its input ring carry gray images only");
  if (UsesRing()) {
    for (int g = 0; g < G_; g++)
      if (!ring_[g]) throw std::runtime_error("input ring: the rings were not allocated (TrackerFarm::SetHostInput)");
    if (!feed_ && sdvl_feed_create(gpu_, G_ * kRingSlots, &feed_) != SDVL_OK) throw std::runtime_error("input ring: sdvl_feed_create failed");
  }
  // everything the threads of the run read is in place before the first of them starts
  n_steps_ = n_steps; stride_ = stride; frames_ = frames; out_ = out;
  sched_.Reset(G_, n_steps, kRingSlots);
  stats_ = FeedStats();
  const char *timeline_path = std::getenv("SDVL_FARM_TIMELINE");
  timeline_ = timeline_path != nullptr;
  step_marks_.assign(timeline_ ? G_ : 0, {});
  feed_marks_.clear();
  if (timeline_ && mark_prev_.size() != static_cast<size_t>(G_)) mark_prev_.assign(G_, std::vector<double>(ST_COUNT, 0.0));
  run_t0_ = std::chrono::steady_clock::now();

  // no exception leaves a thread: what its body throws (a fiber stack that cannot be mapped) fails the run
  auto guarded = [this](auto body) {
    try {
      body();
    } catch (const std::exception &e) {
      sched_.Fail(e.what());
    } catch (...) {
      sched_.Fail("unknown exception in a farm thread");
    }
  };
  std::thread feeder;
  if (UsesRing()) feeder = std::thread([&] { guarded([&] { RunFeeder(); }); });
  static const bool profile = std::getenv("SDVL_PROFILE") != nullptr;
  if (profile) SamplingProfileStart();
  std::vector<std::thread> threads;
  for (int w = 0; w < W; w++)
    threads.emplace_back([&, w] {
      timer_t pt = profile ? SamplingProfileThreadStart() : nullptr;
      guarded([&] {
        if (fibers_per_worker_ > 1) RunShareFibers(w, W);
        else RunShare(w, W);
      });
      SamplingProfileThreadStop(pt);
    });
  for (auto &t : threads) t.join();
  if (feeder.joinable()) feeder.join();  // it has returned or is about to: every step is issued, or the failure woke it
  if (profile) SamplingProfileStopAndPrint();
  if (timeline_) WriteTimeline(timeline_path);
  if (sched_.Failed()) throw std::runtime_error(sched_.Error());
}

}  // namespace sdvl
