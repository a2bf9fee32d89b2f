// sdvl_search_types.h — device records of the search stage (sdvl_search.hip), shared with the device-resident tracking
// tables (sdvl_track.hip), which write them on the device instead of receiving them from the host.
#ifndef SDVL_SEARCH_TYPES_H_
#define SDVL_SEARCH_TYPES_H_

#include "sdvl_internal.h"
#include "sdvl_math.h"

constexpr int kWavesPerBlock = 4;  // requests of one workgroup; they all search the SAME current frame (block table)
constexpr int kLdsCorners = 4096;  // corners of the current frame staged in LDS (16 KB: 8 workgroups per CU); a frame with
                                   // more (up to SDVL_MAX_CORNERS) has the rest read from HBM / L2

struct SearchBlock {
  int first, count;  // requests [first, first + count) of the launch, count <= kWavesPerBlock
};

struct SearchFrame {
  const uint8_t *level[SDVL_MAX_LEVELS];
  int lw[SDVL_MAX_LEVELS], lh[SDVL_MAX_LEVELS];
  const int32_t *corners;
  const uint8_t *desc;
  const int32_t *n_ptr;  // device-resident corner count
  int levels;
  int bin_gw;            // corners binned by 32-px cell of level-0 coordinates (select_pack_kernel), bin_start == null: none
  const int32_t *bin_start;
  const uint2 *bin_entries;
  int bin_cells, pad_;
  int pad2_[2];
};

// bins_pending: the frame's corners (and their bins) are produced by a detection that is queued BEHIND this call and ahead of the
// kernels that will read the view (sdvl_track_align -> sdvl_detect_corners -> sdvl_track_search): the view names the frame's bin
// arrays although the host does not call them valid yet.  sdvl_track_search checks that the detection did come (track_clear_bins).
inline void fill_view(SearchFrame *d, const sdvl_frame *f, bool bins_pending = false) {
  memset(d, 0, sizeof(SearchFrame));
  for (int l = 0; l < f->v.levels; l++) {
    d->level[l] = f->v.level[l];
    d->lw[l] = f->v.lw[l];
    d->lh[l] = f->v.lh[l];
  }
  d->corners = f->v.corners;
  d->desc = f->desc_valid ? f->v.desc : nullptr;  // null: a search computes the descriptors it compares (search_points_kernel)
  d->n_ptr = f->v.corner_hdr;
  d->levels = f->v.levels;
  if (f->bins_valid || (bins_pending && f->bin_cells > 0)) {
    d->bin_start = f->bin_start;
    d->bin_entries = f->bin_entries;
    d->bin_gw = f->bin_gw;
    d->bin_cells = f->bin_cells;
  }
}

// the kernels' camera record (sdvl_math.h) from the public one
inline sdvl::Cam cam_of(const sdvl_camera &c) { return sdvl::Cam{c.width, c.height, c.fx, c.fy, c.u0, c.v0}; }

// (frame, pose) pairs are shared by many requests of a launch: they go into a table, requests carry two indices
struct SearchFramePose {
  SearchFrame f;
  double pose[7];
  double pad_;
};

struct SearchReqDev {
  int cur, ref;  // indices into the SearchFramePose table of the launch
  int level, fixed;
  double px[2], bearing[3];
  double idepth, idepth_std;
  double px0[2];
  uint32_t desc[8];
};

// what the scalar part of SearchPoint (matcher.cc:45-96) leaves for the wave part: one record per request
struct SearchPrep {
  int alive, slevel;
  double pxa[2], pxb[2];        // projected ends of the depth interval (pxb only for epipolar searches)
  double I00, I01, I10, I11;    // inverse of the affine warp (CreatePatch, matcher.cc:330)
  // wave-uniform constants of GetCornersInRange (matcher.cc:139-148, 92-94), computed once by the request's lane; the wave
  // kernel reads the record with scalar loads, so they live in SGPRs instead of 64 copies in VGPRs
  double nx, ny, normdist, xdiff, ydiff, vline, range, range2;
  // the corner bins the search region touches, looked up by the request's lane as well (round 4: in the wave kernel the box, its cell
  // range and the eight bin offsets were ~100 vector instructions every lane repeated for itself).  bin_mode 0: not prepared (no bins,
  // degenerate epipolar line, a region of more than four cell rows or kBinRegionCells cells: the wave kernel decides as before);
  // 1: the region lies outside the image; 2: cell rows 0..3 contribute entries [bin_e0[r], bin_e0[r] + bin_pre[r + 1] - bin_pre[r])
  int bin_mode, bin_pad_;
  int bin_e0[4], bin_pre[4];  // bin_pre[r] = entries of the rows before r + 1 (bin_pre[3] = all of them)
};

// search regions of up to this many 32-px cells go through the corner bins (their corners: ~3.4 per cell); larger ones scan the whole list.
// The bins are 32-px cells of level 0 whatever SDVL.cell_size is; frames of more than 4096 bins have none (sdvl_ctx.hip frame_layout)
constexpr int kBinRegionCells = 320;

struct ChainFrameDev {
  int cand_begin, cand_end;
  int max_matches, rand_begin;
  int obs_begin, pad_;
  double pose[7];
  double pad2_;
};

// ---- second half of FeatureAlign::SelectPoints (feature_align.cc:105-149): candidates come cell by cell in the reference's order; a
// cell's first found candidate is a match; the first max_matches matches are kept.  Two kernels run it — select_matches_kernel
// (sdvl_search.hip: sets of <= 4 trackers) and wave 0 of pose_refine_kernel (sdvl_pose.hip) — with the statements below.
constexpr int kChainMaxCand = 16384;  // candidates of one tracker whose found flags fit the kernels' LDS words (bit k & 63 of word k >> 6)

// what the selection reads and writes besides the observations; frames == nullptr: no selection, the pose jobs come ready-made
struct PoseChainIn {
  const ChainFrameDev *frames;
  const int32_t *cand_req;    // null: candidate k of a tracker was searched with request cand_begin + k (batches built on the device)
  const int32_t *cand_first;  // first candidate of candidate k's cell
  const sdvl_search_res *res;
  const double *req_point;
  sdvl::Cam cam;
  int32_t *n_obs;             // matches kept, per tracker
  int32_t *match_cand;        // may be null: per kept match its candidate index relative to cand_begin, at obs_begin + rank
};

__device__ __forceinline__ int select_request(const PoseChainIn &in, const ChainFrameDev &fr, int k) {
  return in.cand_req ? in.cand_req[fr.cand_begin + k] : fr.cand_begin + k;
}

__device__ __forceinline__ bool select_found(const PoseChainIn &in, const ChainFrameDev &fr, int k) {
  const int r = select_request(in, fr, k);
  return r >= 0 && in.res[r].found != 0;
}

// candidate k (found) is a match when no candidate first..k-1 of its cell has been found
__device__ __forceinline__ bool select_first_of_cell(const unsigned long long *found_words, int first, int k) {
  if (first < 0) first = 0;
  for (int w = first >> 6; w <= (k >> 6); w++) {
    unsigned long long m = found_words[w];
    if (w == (first >> 6)) m &= ~0ull << (first & 63);
    if (w == (k >> 6)) m &= ~(~0ull << (k & 63));
    if (m) return false;
  }
  return true;
}

// the match of candidate k leaves as pose observation `rank` of its tracker (feature_align.cc:132 creates the Feature — bearing =
// Camera::Unproject(px) — SelectInliers reads bearing/z, the point and 1/2^level)
__device__ __forceinline__ void select_emit(const PoseChainIn &in, const ChainFrameDev &fr, int k, int rank, sdvl_pose_obs *obs) {
  const int req = select_request(in, fr, k);
  const sdvl_search_res &r = in.res[req];
  if (in.match_cand) in.match_cand[fr.obs_begin + rank] = k;
  const sdvl::V3 v = sdvl::cam_unproject(in.cam, {r.px[0], r.px[1]});
  sdvl_pose_obs o;
  o.ax = v.x / v.z;
  o.ay = v.y / v.z;
  const double *P = in.req_point + 3 * static_cast<size_t>(req);
  o.px = P[0];
  o.py = P[1];
  o.pz = P[2];
  o.inv_cov = 1.0 / (1 << r.level);
  obs[fr.obs_begin + rank] = o;
}

// ---- rows of the device-resident tracking tables (sdvl_track.hip); the depth filter (sdvl_depth_filter.hip) patches them in place
constexpr int kDeleted = 0x100;                 // sdvl_track_point_stat::status bit
constexpr int kTrash = 0x200;                   // deleted by the mapper: becomes kDeleted at the end of the next step's commit
constexpr int kKeepBits = kDeleted | kTrash;
enum { kFound = 0, kNotFound = 1, kSeen = 2, kUnseen = 3 };  // Point::PointStatus (point.h)
constexpr int kPointMask = SDVL_TRACK_DUPLICATE - 1;

struct TrackPoint {  // device form of sdvl_track_point: the frame pointer replaced by its registry slot
  double P[3];
  double ipx[2];
  double ibearing[3];
  double idepth, idepth_std;
  int32_t ref, pad_;
  int32_t ilevel, fixed;
  int32_t score, n_failed;
  int32_t last_frame;
  int32_t status;  // Point::PointStatus | kDeleted | kTrash
  uint32_t desc[8];
};
static_assert(sizeof(TrackPoint) == sizeof(sdvl_track_point), "upload converts in place");
static_assert(sizeof(sdvl_track_point) == 144, "layout");
struct TrackFeat {  // a feature row of last_frame (sdvl_track_feature)
  double px[2];
  double bearing[3];
  int32_t level;
  int32_t point;
};
static_assert(sizeof(TrackFeat) == sizeof(sdvl_track_feature) && sizeof(TrackFeat) == 48, "layout");

// one tracked step of one tracker, written by sdvl_track_align and read by every kernel of the step (track_project, track_commit,
// and — round 4 — the image alignment itself: image_align_track_kernel builds its features from the table rows, no records in between)
struct TrackJobDev {
  SearchFrame cur;  // view of the new frame
  int tracker, feat_buf;
  int cur_id, last_id;
  int frame_id, max_matches;
  int n_feat, n_points;
  double last_pose[7];
  double pad_;
  const uint8_t *last_level[SDVL_MAX_LEVELS];  // pyramid of last_frame (frame1 of the alignment; same geometry as cur)
  double T0[7];                                // start of the alignment, frame2.pose * frame1.pose^-1 (image_align.cc:66)
  double pad2_;
};

// the set's point rows and the row count per tracker (sdvl_track.hip)
extern "C" TrackPoint *sdvl_track_points_device(sdvl_track_set *set, int *max_points, int *n_trackers);
// for tests: the visiting order the collected step's reprojection left on the device.  Slot k of job j is entry j * stride + k of arrays
// of `capacity` >= n_jobs * stride entries (px, px0: two doubles each): the candidates come first, in visiting order — cand_first (slot
// of the first candidate of k's cell), cand_feat (row of last_frame's feature list), the request's level, px (the point's first
// observation) and px0 (its projection); behind them req_level is -1 and the rest undefined.  One (block_first, block_count) per 4 slots
extern "C" int sdvl_track_read_order(sdvl_ctx *ctx, const sdvl_track_set *set, int n_jobs, int capacity, int32_t *stride, int32_t *cand_first,
                                     int32_t *cand_feat, int32_t *req_level, double *req_px, double *req_px0, int32_t *block_first,
                                     int32_t *block_count);

// ---- launch helpers of sdvl_search.hip for callers whose records already live in HBM (no copies, no wait) --------------
// search_prepare + search_points over n_slots request records (a record with level < 0 is a dead slot) dealt to workgroups
// by the n_blocks entries of d_blocks (a block with count 0 is skipped); d_res receives one result per slot, h_res (may
// be null) the same records in pinned host memory.  binned: every frame searched came out of sdvl_detect_corners
int sdvl_search_launch_device(sdvl_ctx *ctx, int n_slots, const SearchReqDev *d_reqs, const SearchFramePose *d_table,
                              const SearchBlock *d_blocks, int n_blocks, const sdvl_camera *cam, const sdvl_search_params *p,
                              SearchPrep *d_prep, sdvl_search_res *d_res, sdvl_search_res *h_res, bool prepared = false, bool binned = true);
// second half of SelectPoints for n_frames trackers as a launch of its own (sdvl_pose_enqueue_device queues it for sets of <= 4
// trackers; larger sets select inside pose_refine): fills d_jobs and the observations
int sdvl_select_matches_launch(sdvl_ctx *ctx, int n_frames, const PoseChainIn &in, PoseJobDev *d_jobs, sdvl_pose_obs *d_obs);
// ---- and for the entries that queue a kernel of their own behind a search of host requests (sdvl_depth_filter.hip)
// What a search of n requests keeps in the context's result buffers — d_out: results | per-request records of the scalar phase;
// h_out: results — each at the head, so a caller takes the parts it wants behind them from `d` / `h` before sdvl_search_enqueue.
struct SearchOut {
  sdvl_layout d, h;
  sdvl_part<sdvl_search_res> res, h_res;
  sdvl_part<SearchPrep> prep;
  explicit SearchOut(int n) : res(d.take<sdvl_search_res>(n)), h_res(h.take<sdvl_search_res>(n)), prep(d.take<SearchPrep>(n)) {}
};
// everything of sdvl_search_run up to and including the queued copy of the results into h_out (so.h_res); the caller waits.  -> where
// the batch's requests and frame table lie in HBM
extern "C" int sdvl_search_enqueue(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const SearchOut &so,
                                   const SearchReqDev **d_reqs_out = nullptr, const SearchFramePose **d_table_out = nullptr);
// sdvl_search_begin + one sdvl_search_slot pair per request: the batch of sdvl_search_points
extern "C" int sdvl_search_pack_requests(sdvl_ctx *ctx, int n, const sdvl_search_req *reqs);
// sdvl_image_align.hip: the image alignment of a tracked step, features straight from the tracking tables (no records, no wait)
int sdvl_image_align_track_enqueue(sdvl_ctx *ctx, int n_jobs, const TrackJobDev *d_jobs, const TrackPoint *d_points, const TrackFeat *d_feats0,
                                   const TrackFeat *d_feats1, int np, int nfeat_cap, int max_nf, int levels, const sdvl_camera *cam,
                                   const sdvl_align_params *p, sdvl_align_result *d_results, int batch_size);
// batch_size: the capacity of the set the jobs come from (NOT the jobs of this step): it picks the one-wave or four-wave form for the
// set's life, so that a sequence's sums do not change order when a neighbour bootstraps or is lost
// the iteration-budget table of SelectInliers for all match counts up to max_size, resident in HBM (ctx->d_nits)
extern "C" int sdvl_ensure_nits_table(sdvl_ctx *ctx, int npoints_cfg, int max_its, int max_size);

#endif  // SDVL_SEARCH_TYPES_H_
