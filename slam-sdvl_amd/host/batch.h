// batch.h — SDVLBatch, the project's own batch driver: B independent trackers stepping together, one launch per kernel per stage.  It has
// no counterpart in the reference's tree.  sdvl_host.h includes this header at its end, so `#include "sdvl_host.h"` declares it too.
// The class is implemented in the batch*.cc files, one per job; each section below names the file that holds its functions, and each
// piece of state that only one job uses is a nested struct declared in that job's section.
#ifndef SDVL_BATCH_H_
#define SDVL_BATCH_H_

#include "sdvl_host.h"

namespace sdvl {

class DepthJobs;  // depth_jobs.h

// B independent trackers stepping together, one launch per kernel per stage (MI355X-first driver)
class SDVLBatch {
 public:
  SDVLBatch(Device *dev, const std::vector<SDVL *> &trackers, int host_threads);
  ~SDVLBatch();
  // imgs[i] feeds tracker i; stats[i] receives its FrameStats
  void HandleFrames(const std::vector<Image> &imgs, FrameStats *stats);
  // the same with the frames' registered depth images for the trackers that seed from depth (SDVL::SetDepthSeeding): depths is empty or
  // has one entry per tracker, and single entries may be empty (for a tracker that seeds from a stereo pair, SDVL::SetStereoSeeding, the
  // entry is the pair's right image, DEPTH_RIGHT8, read inside the step's ONE sdvl_stereo_depth call).  A depth image is read inside the
  // step's ONE sdvl_depth_seed call only (FinishKeyframes); nothing is copied or kept, and the look-ahead does not need it.
  void HandleFrames(const std::vector<Image> &imgs, const std::vector<DepthImage> &depths, FrameStats *stats);
  // Round 4: a caller that already holds the images of the NEXT step (a sequence from disk, frames resident in HBM) names them before
  // the current step: their pyramids and corner detection — all that depends on the image alone, 45 % of a step's vector instructions —
  // are queued right behind the current step's search / pose chain and run while the host waits for that chain and does its keyframe
  // bookkeeping; the next HandleFrames with these images picks the frames up.  Same kernels on the same inputs: same results.
  // The images must stay valid until that call (device images are aliased).  An unused look-ahead is dropped.
  void SetNextImages(const std::vector<Image> &next);
  // pose stage (RANSAC + refinement) on the device (default) or with the host implementation; process-wide switch,
  // also set by SDVL_POSE_HOST=1 in the environment.  Both produce the same decisions (tests/test_gpu_tracker.py).
  static void SetDevicePose(bool on);
  static bool DevicePose();
  // Device-resident tracking tables (the default): last_frame's features and points
  // stay in HBM, a step is ONE submission and ONE wait, the host keeps rand(), the motion model and the keyframe logic.
  // Off (SDVL_NO_TRACK_TABLES=1 or SetTrackTables(false)): the host assembles every request as before.  Same results.
  static void SetTrackTables(bool on);
  static bool TrackTables();
  // Point objects / Feature lists catch up with the device (called on its own whenever the batch leaves the tracked path)
  void SyncHostState();

 private:
  void ParallelFor(int n, const std::function<void(int)> &fn);
 public:
  StageTimes stage_times;
 private:
  friend class SDVL;
  // ---- batch.cc: worker pool and process-wide switches; what every form of a step shares; what follows the decisions
  Device *dev_;
  std::vector<SDVL *> trk_;
  int threads_;
  // ParallelFor as Frame's batched calls take it (CreateBatch hands the body over by value, FilterCornersEnd by reference)
  std::function<void(int, std::function<void(int)>)> pfor_;
  std::function<void(int, const std::function<void(int)> &)> pfor_ref_;
  struct Step;      // what the stages of one step hand to each other (defined in batch_internal.h)
  struct HostStep;  // Step + the requests and pose jobs of the host-driven form (defined in batch_host_step.cc)
  enum FrameStart { kFirstFrame, kLost, kRunning };
  FrameStart BeginFrame(int i, const std::shared_ptr<Frame> &frame, FrameStats &st);
  // the two-frame initialisation of every tracker of the step that is in its first-frame or second-frame state: ONE sdvl_klt_track
  // call and ONE sdvl_homography_ransac call for all of them
  void InitializeTrackers(Step &s);
  void DetectOnSideStream(const std::vector<std::shared_ptr<Frame>> &frames, bool fork);
  void FetchCornerCounts(const std::vector<std::shared_ptr<Frame>> &frames, FrameStats *stats);
  void CollectKeyframes(Step &s, bool fetch_counts);
  void EpilogueAndMapper(Step &s);
  void FinishKeyframes(Step &s);
  // ---- batch_depth.cc: the calls of a step that read a frame's second image (depth image, right image), ONE call for all trackers each
  struct MapStep;  // what the stages of the mappers' update hand to each other (defined in batch_internal.h)
  void SeedKeyframesFromDepth(Step &s, std::vector<const double *> *z, std::vector<const uint8_t *> *status);
  void MeasureKeyframeCorners(MapStep &m, const std::vector<char> &need);
  void LookupKeyframeFeatures(MapStep &m);
  void SearchFilterMeasured(MapStep &m, int total, const sdvl_camera &cam, const sdvl_search_params &sp);
  std::vector<int32_t> MeasureCorners(const DepthJobs &jobs, const std::vector<int32_t> &xyl);  // sdvl_stereo_depth or sdvl_depth_seed over filled jobs
  const std::vector<DepthImage> *step_depths_ = nullptr;  // the depth images of the step in flight (HandleFrames, batch.cc)
  const DepthImage *DepthOf(int i);                        // tracker i's, null: none; of a tracker fed raw pairs, the rectified right image
  // SDVL::SetStereoRectification: the raw right images of the step, rectified into HBM by ONE sdvl_rectify call the first time a consumer
  // asks for one (a step without a consumer rectifies nothing)
  void RectifyRights();
  std::vector<DepthImage> rectified_rights_;
  bool rights_rectified_ = false;
  void *d_rights_ = nullptr;
  size_t d_rights_bytes_ = 0;
  struct CameraAndLens {  // the camera of the batch as the device calls take it, and its lens if it has one
    sdvl_camera cam;
    sdvl_distortion dist;
    bool has_lens;
    const sdvl_distortion *lens() const { return has_lens ? &dist : nullptr; }
  };
  CameraAndLens BatchCamera() const;
  std::vector<double> depth_z_;  // the results of the last of those calls; its owners' ranges are handed on as pointers into them
  std::vector<uint8_t> depth_status_;
  void SizeDepthResults(int n);
  // ---- batch_mapper.cc: SDVL::Mapping() of sequential mode for the trackers that own a real mapper, in stages over a MapStep
  void RunMappers();
  bool CollectMappers(MapStep &m);
  void SetUpMeasuring(MapStep &m);
  void PackAndSearch(MapStep &m, bool filter);
  void CandidatePasses(MapStep &m);
  void KeyframePasses(MapStep &m);
  void BundleWindows(MapStep &m);
  // ---- batch_tables.cc: the device-resident tracking tables.  The set and the rows on their way to it; besides the table functions
  // the tabled step (batch_tracked.cc) uses them, batch.cc where it releases the set and appends a keyframe's seeds (FinishKeyframes),
  // and the mappers' stage where it lets the depth filter patch the rows (PackAndSearch)
  struct Tables {
    sdvl_track_set *set = nullptr;
    int cells = 0, cap = 0;
    std::vector<sdvl_track_job> jobs;   // the tabled step's inputs and results, reused from step to step
    std::vector<uint16_t> rank;
    std::vector<int32_t> rand;
    std::vector<sdvl_track_result> res;
    std::vector<sdvl_track_point> up_points;  // GatherRows: the rows of one upload / append
    std::vector<sdvl_track_feature> up_feats;
    std::vector<int32_t> up_trk, up_buf, up_np, up_nf;  // whose rows those are, for which buffer, how many
  } tables_;
  void SyncStats(SDVL &t);
  bool BuildTable(SDVL &t);
  bool AppendSeeds(SDVL &t, const std::shared_ptr<Frame> &kf);  // rows of the points seeded on kf -> track_.up_points / up_feats
  void GatherRows(const std::vector<int> &up, bool own_buf);
  bool UploadTables(const std::vector<int> &need, std::vector<char> *built);
  bool EnsureTrackSet();
  void InvalidateStaleTables();
  // ---- batch_tracked.cc: the step on the device-resident tables
  bool HandleFramesTracked(const std::vector<Image> &imgs, FrameStats *stats);  // false: not applicable this step
  bool TrackedStepApplies();
  void TakeLookAhead(Step &s);
  void QueueLookAhead(const Step &s);
  void RelocalizeIntoStep(Step &s);
  sdvl_track_params AssembleTrackJobs(const Step &s);
  void SubmitTracked(Step &s);
  void ReplayTracked(Step &s);
  void SaveTrackedFrames(Step &s);
  int TrackOnHost(SDVL &t, FrameStats *st);
  // the look-ahead; HandleFrames (batch.cc) drops it when the step leaves the tables
  std::vector<Image> next_imgs_;                        // SetNextImages: what the next step will be given
  std::vector<std::shared_ptr<Frame>> ahead_frames_;    // their frames, pyramids and detection queued
  std::vector<const void *> ahead_src_;                 // the images they were made from
  // ---- batch_reloc.cc: relocalisation inside the tabled step
  void RelocalizeLost(const std::vector<int> &lost, FrameStats *stats, std::vector<char> *found);
  void PackRelocCache(SDVL &t, std::vector<sdvl_align_feature> *packed);
  void RefreshRelocStore(const std::vector<int> &lost);
  void RelocAlignKeyframes(const std::vector<int> &lost, std::vector<int> *first, std::vector<sdvl_align_result> *res);
  void RelocAlign(const std::vector<sdvl_align_job> &jobs, const sdvl_align_params &ap, std::vector<sdvl_align_result> *res);
  // keyframe feature records of the trackers that are relocalising (SDVL::RelocCache): one bump-allocated store per batch, released with
  // the batch.  Only batch_reloc.cc names its members (and the constructor in batch.cc, which hands it the device).
  struct RelocStore {
    Device *dev;
    sdvl_align_store *store = nullptr;
    int cap = 0, used = 0;
    unsigned long long epoch = 0;  // 0: no store yet
    ~RelocStore();
  } reloc_store_;
  // ---- batch_host_step.cc: the host-driven step
  void HandleFramesGeneric(const std::vector<Image> &imgs, FrameStats *stats);
  bool RelocalizeOnHost(SDVL &t, FrameStats &st);
  void AlignImages(HostStep &s);
  void PackRequests(HostStep &s);
  void PackChain(HostStep &s);
  void CollectRequests(HostStep &s);
  void LaunchSearch(HostStep &s);
  void ReplaySelect(HostStep &s);
  void LaunchPose(HostStep &s);
  void CommitAndSave(HostStep &s);
  // per-step request / pose batches of the stages above, reused so that they never reallocate.  Only batch_host_step.cc names it.
  struct HostScratch {
    std::vector<sdvl_search_req> reqs;
    FeatureAlign::PoseBatch pose;
    std::vector<double> points;  // sdvl_search_run_chain inputs, same idea
    std::vector<int32_t> cand_req, cand_first, rand;
  } host_scratch_;
};

}  // namespace sdvl

#endif  // SDVL_BATCH_H_
