// farm.h — many trackers on one MI355X, for C++ callers and, through capi.cc, for the Python harness.
//   TrackerGroup: B trackers stepping together on one Device — a Camera, a map and an SDVL each, and their SDVLBatch.
//   TrackerFarm:  G groups x Bg sequences on ONE GPU.  Every group owns an sdvl::Device (= sdvl_ctx = HIP stream + staging + frame
//                 pool) and a TrackerGroup; groups free-run through their steps on worker threads, so the host stages of one group
//                 overlap the kernels and PCIe copies of the others (one context per host thread, as include/sdvl_hip.h prescribes).
// Which group steps next, and what the threads of a run tell each other, is farm_schedule.h.
#ifndef SDVL_FARM_H_
#define SDVL_FARM_H_

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "farm_schedule.h"
#include "sdvl_host.h"

namespace sdvl {

class TrackerGroup {
 public:
  // where the images of a step live
  enum class Frames {
    kHost,       // host pointers: every frame uploads its image inside the step
    kResident,   // device pointers that stay valid while the trackers may still read them (the last frame and every keyframe keep their
                 // level 0): aliased, not copied
    kTransient,  // device pointers valid for THIS step only (a slot of an input ring): aliased while tracked; the frames that become
                 // keyframes copy their image out at the end of the step (Frame::OwnImages).  The caller must not refill the buffer
                 // before work queued on the batch's stream has passed
  };

  // use_mapper: every tracker owns the reference's mapper in sequential mode (map.cc) instead of the plane map stub (every keyframe seeded
  // from the scene plane); the first keyframe is bootstrapped from the plane in both modes
  TrackerGroup(Device *dev, int B, int w, int h, const double *cam4, const double *plane4, const double *first_poses7, int host_threads,
               bool use_mapper);
  ~TrackerGroup();
  TrackerGroup(const TrackerGroup &) = delete;
  TrackerGroup &operator=(const TrackerGroup &) = delete;

  // imgs[i] (row stride `stride`, in bytes) feeds tracker i; out[i] receives its FrameStats
  void Step(Frames where, const void *const *imgs, int stride, FrameStats *out);
  // the same with the frames' registered depth images (SetDepth): depths[i] feeds tracker i — host pointers with kHost, device pointers
  // otherwise, dense rows of the format SetDepth named; depths or single entries may be null
  void Step(Frames where, const void *const *imgs, int stride, const void *const *depths, FrameStats *out);
  // Look-ahead (SDVLBatch::SetNextImages): the device images the NEXT Step(kResident) will be given (null: none); their pyramids and corner
  // detection are queued behind the coming step's search / pose chain.  They must stay valid AND UNCHANGED until that call: the look-ahead
  // is matched to the next step's images by device address alone, so a buffer that is rewritten in between would be tracked from pyramids
  // of its old content.  The look-ahead belongs to the one coming step: if that step cannot use it (a bootstrap step, the host-driven
  // path) it is dropped.
  void SetNextImages(const void *const *dev_imgs, int stride);

  // The camera gets a lens (Camera::SetDistortions, camera.cc:39-67; dist5 = Camera.d1..d5 of the cfg files) and the images of every later
  // step are taken as RAW camera frames: Camera::UndistortImage (main.cc:133) runs inside the step, fused into the frames' upload.
  // dist5[0] == 0 (the reference's test, camera.cc:46) turns it off again.
  void SetDistortion(const double *dist5);
  // The images of every later step are COLOUR camera frames of `format` (enum sdvl_pixel_format; row strides in bytes): cv::cvtColor
  // (video_source.cc:63) runs on the device inside the step, fused into the frames' upload, before the undistortion of a lens.  SDVL_RGB8
  // is what main.cc computes on cv::VideoCapture's bytes; SDVL_GRAY8 (0) turns it off again.  RAW camera formats (enum sdvl_raw_format:
  // Bayer mosaics, YUYV / UYVY, 16-bit gray) are converted the same way; row strides are width x bytes per pixel.  Throws on an unknown format.
  void SetColor(int format);
  // Depth cameras (SDVL::SetDepthSeeding for every tracker): keyframes are seeded from the depth images handed to Step, which are of
  // `format` (DEPTH_F32 / DEPTH_U16) with `scale` metres per unit.  Throws what SDVL::SetDepthSeeding throws, and on an unknown format
  // or a scale <= 0 with DEPTH_U16.
  void SetDepth(bool on, int format, double scale, const sdvl_depth_seed_params &rule);
  // Stereo cameras (SDVL::SetStereoSeeding for every tracker): the second images handed to Step are the pairs' rectified right images,
  // 8-bit gray with dense rows.  Throws what SDVL::SetStereoSeeding throws.
  void SetStereo(bool on, double baseline, const sdvl_stereo_params &rule);
  // Stereo cameras inside the mappers (SDVL::SetStereoMapping for every tracker; the trackers share disparity_sigma).  Throws what it throws.
  void SetStereoMapping(bool on, double disparity_sigma = 0.0);
  // Stereo rigs as calibrated (SDVL::SetStereoRectification for every tracker): the images and the second images handed to Step are the
  // RAW images of the rig's two cameras; the group's camera must be the pair's rectified camera.  Throws what it throws.
  void SetStereoRectification(const RectifiedPair &pair, bool on = true);

  Device *device() const { return dev_; }
  int size() const { return static_cast<int>(trackers_.size()); }
  int width() const { return w_; }
  int height() const { return h_; }
  SDVL &tracker(int i) const { return *trackers_[i]; }
  PlaneMap &map(int i) const { return *maps_[i]; }
  SDVLBatch &batch() const { return *batch_; }

 private:
  std::vector<Image> Wrap(Frames where, const void *const *imgs, int stride) const;

  Device *dev_;
  int w_, h_;
  std::unique_ptr<Camera> cam_;
  std::vector<std::unique_ptr<PlaneMap>> maps_;
  std::vector<std::unique_ptr<SDVL>> trackers_;
  std::unique_ptr<SDVLBatch> batch_;
  bool raw_input_ = false;  // SetDistortion: the images of a step are RAW camera frames (Image::raw)
  int format_ = PIX_GRAY8;  // SetColor: the pixel format of the images of a step
  int depth_format_ = DEPTH_F32;  // SetDepth: the depth images of a step
  double depth_scale_ = 1.0;
};

class TrackerFarm {
 public:
  // first_poses7: [G * Bg][7], group-major.  Sets the process's malloc parameters for G allocating threads (farm.cc).
  TrackerFarm(int gpu, int G, int Bg, int w, int h, const double *cam4, const double *plane4, const double *first_poses7,
              int host_threads_per_group, bool use_mapper);
  ~TrackerFarm();
  TrackerFarm(const TrackerFarm &) = delete;
  TrackerFarm &operator=(const TrackerFarm &) = delete;

  int groups() const { return G_; }
  Device &device(int g) const { return *devices_[g]; }
  TrackerGroup &group(int g) const { return *groups_[g]; }

  // pool `frames_per_group` free HBM frames in every group (keyframe budget), so the run allocates nothing
  void Reserve(int frames_per_group);
  // n > 1: every worker thread interleaves n group-steps and switches between them at GPU waits (0 / 1 = one at a time)
  void SetFibers(int n);
  // the frame pointers handed to Run are host pointers (SDVL::HandleFrame(const cv::Mat&) takes a host image, sdvl.cc:55-59)
  void SetHostInput(bool on);
  // the input ring of host-fed runs on (default) / off (every step uploads its own frames on its own stream before it computes)
  void SetInputRing(bool on) { input_ring_ = on; }
  // every group's frames are colour or raw camera frames of `format` (TrackerGroup::SetColor).  Formats of more than one byte per pixel
  // must be resident in HBM: the host input and its input ring (sdvl_feed_*) carry one byte per pixel, and Run refuses the combination.
  // The four Bayer formats are one byte per pixel: they ride the ring and the ring-less host path as the gray bytes they are, and are
  // converted inside the step.
  void SetColor(int format);

  // Runs n_steps steps with `workers` host threads (0 = one per group).  frames[(step * G*Bg) + g*Bg + i] = pointer to the frame of
  // sequence (g, i) at that step (row stride = `stride`); out[(step * G*Bg) + g*Bg + i] receives its stats.  Throws std::runtime_error
  // with the first failure of the run.
  void Run(int n_steps, const void *const *frames, int stride, FrameStats *out, int workers);

  // the last host-fed run
  struct FeedStats {
    double feed_call_s = 0.0;      // the feeder's time inside sdvl_feed_images
    double feed_wait_s = 0.0;      // ... waiting for a free ring slot
    long feed_calls = 0;           // transfers
    double work_wait_s = 0.0;      // the workers' time waiting for their step's transfer to be issued (summed over groups)
    double arrive_wait_s = 0.0;    // ... and for it to arrive (host-side polls, summed over groups)
    long late_acquires = 0;        // group-steps that began while their transfer was still under way
    double feed_throttle_s = 0.0;  // the feeder's time waiting for its own earlier transfers (at most two are queued on the device)
  };
  FeedStats feed_stats() const;

 private:
  struct Fiber;
  struct FiberScheduler;
  static thread_local FiberScheduler *fiber_sched_;  // of the worker thread that is running fibers
  static void FiberWaitHook(void *, sdvl_ctx *ctx);
  static void FiberMain(unsigned lo, unsigned hi);

  bool UsesRing() const { return host_input_ && input_ring_; }
  void *RingSlot(int g, int s) const;  // where the images of step s of group g travel to: Bg frames, one after the other
  int StepGroup(int g, int s, std::string *message) noexcept;
  void StepGroupOnRing(int g, int s, FrameStats *out);
  bool StepAndFinish(int g, int s);
  void RunFeeder();
  void RunShare(int worker, int n_workers);
  void RunShareFibers(int worker, int n_workers);
  void WriteTimeline(const char *path) const;
  double Since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - run_t0_).count(); }

  // Host input travels ahead: while a group computes step s, the images of its next steps travel into the free slots of the group's
  // input ring (kRingSlots x Bg frames of HBM).  ONE copy stream for the whole farm, filled by a feeder thread of its own (sdvl_feed), and a
  // ring of three steps per group.  Before, every group's worker thread issued its own prefetch on its own copy stream: hipMemcpyAsync of
  // 79 MB kept the worker for a good part of the transfer (15 of the 34 ms of a group-step were spent outside HandleFrames), and the 16
  // groups' transfers ran side by side and shared the link, so the one a group was waiting for was slowed by the ones nobody needed yet
  // (38-47 GB/s of the 57 the link gives; a ring of three was slower still).  The feeder issues the transfers one after the other, the
  // group that is furthest behind first; the workers only exchange events with it.
  static constexpr int kRingSlots = 3;
  // SDVL_FARM_TIMELINE=<file>: one line per group-step (group, step, enter, transfer issued, step returned, late, keyframes, the step's
  // share of the first kTimelineStages stage clocks) and per transfer (group, step, call begin, call end), seconds since the run began
  static constexpr int kTimelineStages = 12;
  static_assert(kTimelineStages <= ST_COUNT, "the timeline's stage columns are the first StageIds");
  struct StepMark { int g, s; double t_enter, t_issued, t_end; int late; double st[kTimelineStages]; int kf; };
  struct FeedMark { int g, s; double t0, t1; };

  const int gpu_, G_, Bg_, w_, h_;
  // destroyed in this order: groups, feed, rings, devices (~TrackerFarm)
  std::vector<std::unique_ptr<Device>> devices_;
  std::vector<std::unique_ptr<TrackerGroup>> groups_;
  std::vector<void *> ring_;  // [group] HBM of the group's input ring, on its device
  sdvl_feed *feed_ = nullptr;

  int format_ = PIX_GRAY8;
  int fibers_per_worker_ = 1;
  bool host_input_ = false;
  bool input_ring_ = true;

  // the current run
  FarmSchedule sched_;
  int n_steps_ = 0, stride_ = 0;
  const void *const *frames_ = nullptr;
  FrameStats *out_ = nullptr;
  std::chrono::steady_clock::time_point run_t0_;
  std::mutex stats_m_;  // arrive_wait_s, late_acquires: written by every worker
  FeedStats stats_;
  bool timeline_ = false;
  std::vector<std::vector<StepMark>> step_marks_;  // [group], written by the thread that steps the group
  std::vector<FeedMark> feed_marks_;               // written by the feeder
  std::vector<std::vector<double>> mark_prev_;     // [group] the stage clocks at the group's previous mark
};

}  // namespace sdvl

#endif  // SDVL_FARM_H_
