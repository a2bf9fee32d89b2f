// sdvl_track.hip — device-resident tracking tables: what FeatureAlign::Reproject reads every frame (the features of
// last_frame and the points behind them) lives in HBM, and the per-frame work the host used to do around the kernels —
// ProjectPoints, the grid, the per-cell sort by score, request assembly (feature_align.cc:88-150,285-339), the replay of
// SelectPoints' bookkeeping (Promote / Unpromote / MaxFailed), RemoveOutliers (:245-256) and the new frame's feature list —
// runs in three small kernels around the existing ones:
//
//   [image_align]      sdvl_image_align.hip, results stay in HBM
//   track_project      pose = T * last_pose; ProjectPoints; candidates ordered as SelectPoints visits them (cell by cell in
//                      the caller's shuffled order, inside a cell by score, stable) -> request records, cell starts, block
//                      table, the pose stage's frame record; the (frame, pose) registry entry of the new frame
//   [search_prepare, search_points, select_matches, pose_hypotheses, pose_refine]
//   track_commit       which candidates SelectPoints would have tried; Promote / Unpromote / delete; the matches become the
//                      new frame's features (other buffer); outliers lose their point; results + mirrors to pinned host memory
//
// One workgroup per tracker in the three kernels; nothing here needs a workgroup-to-workgroup hand-off.
// Compiled with -ffp-contract=off like everything else: the arithmetic is the host layer's, statement for statement.
#include <atomic>
#include <chrono>
#include <vector>

#include "sdvl_internal.h"
#include "sdvl_math.h"
#include "sdvl_search_types.h"
#include "sdvl_search_prepare.h"
#include "sdvl_wave.h"

namespace {

using namespace sdvl;


struct UploadRec {  // sdvl_track_upload / sdvl_track_append: where one tracker's staged rows go
  int tracker, feat_buf;
  int n_points, n_feat;
  long long point_off, feat_off;  // element offsets into the staged arrays
  int point_dst, feat_dst;        // first row written in the tracker's tables (0: the table is replaced; > 0: rows are appended)
  long long pad_;
};

struct RegisterRec {  // sdvl_frame_register
  SearchFramePose e;
  int id, pad_;
};

// the rare case behind fill_view's bins_pending: current frames whose corners did not come out of sdvl_detect_corners (set by hand)
// have no bins: their views go back to "scan the whole corner list"
__global__ __launch_bounds__(64) void track_clear_bins_kernel(TrackJobDev *__restrict__ jobs, const uint8_t *__restrict__ no_bins, int n) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j < n && no_bins[j]) {
    jobs[j].cur.bin_start = nullptr;
    jobs[j].cur.bin_entries = nullptr;
    jobs[j].cur.bin_gw = 0;
    jobs[j].cur.bin_cells = 0;
  }
}

__global__ __launch_bounds__(64) void registry_write_kernel(const RegisterRec *__restrict__ recs, int n, SearchFramePose *__restrict__ registry) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) registry[recs[i].id] = recs[i].e;
}

__global__ __launch_bounds__(256) void track_upload_kernel(const UploadRec *__restrict__ recs, const TrackPoint *__restrict__ src_points,
                                                           const TrackFeat *__restrict__ src_feats, TrackPoint *__restrict__ points,
                                                           TrackFeat *__restrict__ feats0, TrackFeat *__restrict__ feats1, int np, int nf) {
  const UploadRec r = recs[blockIdx.x];
  // rows are multiples of 16 bytes: copy them as such
  const uint4 *sp = reinterpret_cast<const uint4 *>(src_points + r.point_off);
  uint4 *dp = reinterpret_cast<uint4 *>(points + static_cast<size_t>(r.tracker) * np + r.point_dst);
  const int pw = r.n_points * static_cast<int>(sizeof(TrackPoint) / 16);
  for (int i = threadIdx.x; i < pw; i += 256) dp[i] = sp[i];
  const uint4 *sf = reinterpret_cast<const uint4 *>(src_feats + r.feat_off);
  uint4 *df = reinterpret_cast<uint4 *>((r.feat_buf ? feats1 : feats0) + static_cast<size_t>(r.tracker) * nf + r.feat_dst);
  const int fw = r.n_feat * static_cast<int>(sizeof(TrackFeat) / 16);
  for (int i = threadIdx.x; i < fw; i += 256) df[i] = sf[i];
}

constexpr int kProjThreads = 512;
constexpr int kProjOneWaveStride = 512;  // a farm's sets project with one wave up to this stride (8 rounds of 64 features)
// track_project orders a job's candidates through a histogram over the cell ranks (one bucket per cell and one, the last, for the rank
// 0xFFFF of projections outside the grid) for grids of up to this many cells; larger grids (sdvl_track_create takes up to 65535 cells)
// keep the quadratic count of smaller keys.  2048 cells: 4 KB of histogram, so that stride 2048 stays below the default LDS limit
// (53312 + 4100 bytes); 640x480 at cell 32 has 300 cells, configuration C's 1280x960 1200, 1920x1080 2040
constexpr int kProjBuckets = 2048;

// dynamic LDS of track_project_kernel for `stride` feature slots on a grid of `cells` cells — s_key [stride] 64-bit at 0 | s_px
// [stride][2] doubles | s_cell [stride] 16-bit (the histogram form's s_seg lies there: it has no use for s_cell) | s_hist [cells + 1]
// 16-bit in 32-bit words (none beyond kProjBuckets cells) | 64 spare: byte offsets of the parts and the total
struct ProjLds {
  size_t px, cell, hist, bytes;
  __host__ __device__ constexpr ProjLds(size_t stride, size_t cells)
      : px(8 * stride), cell(px + 16 * stride), hist(cell + 2 * stride),
        bytes(hist + (cells <= static_cast<size_t>(kProjBuckets) ? 4 * ((cells + 2) / 2) : 0) + 64) {}
};
constexpr size_t kProjLdsDefault = 60 * 1024, kProjLdsMax = ProjLds(4096, kProjBuckets).bytes;  // beyond the first the limit is raised, to the largest set's (<= 4096 features)
static_assert(kProjLdsMax == 110660, "track_project at stride 4096");
static_assert(ProjLds(2048, kProjBuckets).bytes <= kProjLdsDefault, "stride 2048 (the alignment's limit) within the default");

// inclusive prefix sum over the 64 lanes (all active): wave_sum_i32's steps (sdvl_wave.h) without the final readlane — a scan inside the
// 16-lane rows, then the two row broadcasts
__device__ __forceinline__ int wave_scan_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xe, false);  // row_shr:4, banks 1-3
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xc, false);  // row_shr:8, banks 2-3
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return v;
}

// hand-off through LDS between the phases of track_project: a workgroup of one wave needs no s_barrier
template <bool kOneWave>
__device__ __forceinline__ void proj_sync() {
  if constexpr (kOneWave) wave_sync();
  else __syncthreads();
}

// ProjectPoints + the first half of SelectPoints (feature_align.cc:88-118,285-339).  kOneWave: launched with 64 threads (a farm's sets)
template <bool kOneWave>
__global__ __launch_bounds__(kOneWave ? 64 : kProjThreads) void track_project_kernel(const TrackJobDev *__restrict__ jobs, TrackPoint *__restrict__ points,
                                                                     const TrackFeat *__restrict__ feats0, const TrackFeat *__restrict__ feats1,
                                                                     int np, int nf, int stride, int mm, int max_its,
                                                                     const sdvl_align_result *__restrict__ ares,
                                                                     const uint16_t *__restrict__ cell_rank, int cells, Cam cam, int cell_size,
                                                                     int patch, SearchFramePose *__restrict__ registry,
                                                                     SearchReqDev *__restrict__ reqs, double *__restrict__ req_point,
                                                                     int32_t *__restrict__ cand_first, int32_t *__restrict__ cand_feat,
                                                                     SearchBlock *__restrict__ blocks, ChainFrameDev *__restrict__ chain,
                                                                     sdvl_search_params sprm, SearchPrep *__restrict__ prep) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  const ProjLds lds(stride, cells);
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(s_dyn);  // [stride] sort key of feature i, ~0 = not a candidate
  double *s_px = reinterpret_cast<double *>(s_dyn + lds.px);                   // [stride][2] its projection
  uint16_t *s_cell = reinterpret_cast<uint16_t *>(s_dyn + lds.cell);           // [stride] cell of the candidate at sorted position k (quadratic form)
  uint16_t *s_seg = s_cell;                                                    // [stride] histogram form: candidates bucket by bucket, any order inside one
  unsigned *s_hist = reinterpret_cast<unsigned *>(s_dyn + lds.hist);           // [cells + 1] 16-bit, two to a word: count, then start, then end of a bucket
  __shared__ double s_pose[7];
  __shared__ int s_ncand;
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int nthreads = kOneWave ? 64 : static_cast<int>(blockDim.x);
  const TrackJobDev &jb = jobs[j];
  const TrackFeat *F = (jb.feat_buf ? feats1 : feats0) + static_cast<size_t>(jb.tracker) * nf;
  TrackPoint *P = points + static_cast<size_t>(jb.tracker) * np;
  const int n_feat = jb.n_feat;
  const int base = j * stride;
  const bool linear = cells <= kProjBuckets;     // visiting positions through the histogram
  const int hist_words = linear ? (cells + 2) / 2 : 0;
  if (tid == 0) {
    // frame2.pose = T * frame1.pose (image_align.cc:79)
    const Rigid pose = se3_mul(se3_from7(ares[j].T), se3_from7(jb.last_pose));
    se3_to7(pose, s_pose);
    s_ncand = 0;
    SearchFramePose e;
    e.f = jb.cur;
    se3_to7(pose, e.pose);
    e.pad_ = 0.0;
    registry[jb.cur_id] = e;
  }
  for (int w = tid; w < hist_words; w += nthreads) s_hist[w] = 0u;
  proj_sync<kOneWave>();
  const Rigid pose = se3_from7(s_pose);
  const M3 R = se3_rot(pose);
  // the FeatureAlign grid: cell ranks are 16-bit (sdvl_track_create: <= 65535 cells); 3840x2160 at cell 32 has 8160, at 8 px 130 k are refused there
  const int gw = static_cast<int>(ceil(cam.width / cell_size));
  int n_cand = 0;
  for (int i0 = 0; i0 < n_feat; i0 += nthreads) {  // (whole waves go round: the ballot below)
    const int i = i0 + tid;
    unsigned long long key = ~0ull;
    if (i < n_feat) {
      const int praw = F[i].point;
      if (praw >= 0 && !(praw & SDVL_TRACK_DUPLICATE)) {
        TrackPoint &p = P[praw];
        if (!(p.status & kDeleted) && p.last_frame != jb.frame_id) {
          // ProjectPoint, feature_align.cc:317-339; Frame::Project, frame.cc:94-103
          const V3 rel = vadd(mvec(R, {p.P[0], p.P[1], p.P[2]}), pose.t);
          bool ok = !(rel.z < 0.0);
          V2 px = {0.0, 0.0};
          if (ok) {
            px = cam_project(cam, rel);
            ok = cam_inside(cam, static_cast<int>(px.x), static_cast<int>(px.y), patch);
          }
          if (!ok) {
            p.status = (p.status & kTrash) | kUnseen;
          } else {
            const int k = static_cast<int>(px.y / cell_size) * gw + static_cast<int>(px.x / cell_size);
            const unsigned sc = static_cast<unsigned>(p.score < 0 ? 0 : (p.score > 0xFFFFFF ? 0xFFFFFF : p.score));
            // cells in the shuffled order; inside a cell by descending score, ties in list order (std::list::sort is stable)
            const unsigned rank = k < cells ? cell_rank[static_cast<size_t>(j) * cells + k] : 0xFFFFu;
            key = (static_cast<unsigned long long>(rank) << 48) | (static_cast<unsigned long long>(0xFFFFFFu - sc) << 24) | static_cast<unsigned>(i);
            if (linear) {
              const unsigned b = rank == 0xFFFFu ? static_cast<unsigned>(cells) : rank;
              atomicAdd(&s_hist[b >> 1], 1u << (16 * (b & 1)));  // (a count is at most stride <= 4096: nothing carries into the neighbour)
            }
            s_px[2 * i] = px.x;
            s_px[2 * i + 1] = px.y;
            p.status = (p.status & kTrash) | kSeen;
          }
          p.last_frame = jb.frame_id;  // not relocalising (the tables are only used for ordinary tracking)
        }
      }
      s_key[i] = key;
    }
    const unsigned long long is_cand = __ballot(key != ~0ull);
    if constexpr (kOneWave) n_cand += __popcll(is_cand);
    else if (lane == 0 && is_cand) atomicAdd(&s_ncand, __popcll(is_cand));
  }
  proj_sync<kOneWave>();
  if constexpr (!kOneWave) n_cand = s_ncand;
  if (linear) {
    // exclusive prefix over the buckets in bucket order, by the first wave: a lane takes a word (two buckets), 128 buckets a round
    if (tid < 64) {
      int carry = 0;
      for (int w0 = 0; w0 < hist_words; w0 += 64) {
        const int w = w0 + lane;
        const unsigned word = w < hist_words ? s_hist[w] : 0u;
        const int lo = static_cast<int>(word & 0xFFFFu), both = lo + static_cast<int>(word >> 16);
        const int incl = wave_scan_i32(both);
        const int start = carry + incl - both;
        if (w < hist_words) s_hist[w] = static_cast<unsigned>(start) | (static_cast<unsigned>(start + lo) << 16);
        carry += __builtin_amdgcn_readlane(incl, 63);
      }
    }
    proj_sync<kOneWave>();
    // every candidate into its bucket's segment; the bucket's start moves up to its end
    for (int i = tid; i < n_feat; i += nthreads) {
      const unsigned long long key = s_key[i];
      if (key == ~0ull) continue;
      const unsigned rank = static_cast<unsigned>(key >> 48), b = rank == 0xFFFFu ? static_cast<unsigned>(cells) : rank;
      const unsigned before = atomicAdd(&s_hist[b >> 1], 1u << (16 * (b & 1)));
      s_seg[(before >> (16 * (b & 1))) & 0xFFFFu] = static_cast<uint16_t>(i);
    }
    proj_sync<kOneWave>();
  }
  // position of every candidate in visiting order = number of smaller keys (keys are unique: they end in the feature index)
  for (int i = tid; i < n_feat; i += nthreads) {
    const unsigned long long key = s_key[i];
    if (key == ~0ull) continue;
    int r = 0;
    if (linear) {
      // = candidates in buckets of smaller rank + smaller keys of its own bucket
      const unsigned rank = static_cast<unsigned>(key >> 48), b = rank == 0xFFFFu ? static_cast<unsigned>(cells) : rank;
      const unsigned below = b ? b - 1 : 0;
      const int first = b ? static_cast<int>((s_hist[below >> 1] >> (16 * (below & 1))) & 0xFFFFu) : 0;
      const int end = static_cast<int>((s_hist[b >> 1] >> (16 * (b & 1))) & 0xFFFFu);
      r = first;
      for (int q = first; q < end; q++) r += s_key[s_seg[q]] < key ? 1 : 0;
      cand_first[base + r] = base + first;
    } else {
      for (int q = 0; q < n_feat; q++) r += s_key[q] < key ? 1 : 0;
      s_cell[r] = static_cast<uint16_t>(key >> 48);
    }
    const TrackPoint &p = P[F[i].point];
    SearchReqDev rq;
    rq.cur = jb.cur_id;
    rq.ref = p.ref;
    rq.level = p.ilevel;
    rq.fixed = p.fixed;
    rq.px[0] = p.ipx[0]; rq.px[1] = p.ipx[1];
    rq.bearing[0] = p.ibearing[0]; rq.bearing[1] = p.ibearing[1]; rq.bearing[2] = p.ibearing[2];
    rq.idepth = p.idepth;
    rq.idepth_std = p.idepth_std;
    rq.px0[0] = s_px[2 * i]; rq.px0[1] = s_px[2 * i + 1];
#pragma unroll
    for (int w = 0; w < 8; w++) rq.desc[w] = p.desc[w];
    reqs[base + r] = rq;
    // phase 0 of SearchPoint for the request this lane has just assembled (search_prepare_kernel's work, sdvl_search_prepare.h);
    // the reference frame's pose comes out of the registry, the current frame's is the one this workgroup has just computed
    if (prep) prep[base + r] = search_prepare_one(rq, pose, se3_from7(registry[p.ref].pose), cam, sprm, &jb.cur);  // (the bins were filled earlier in this stream)
    double *rp = req_point + 3 * static_cast<size_t>(base + r);
    rp[0] = p.P[0]; rp[1] = p.P[1]; rp[2] = p.P[2];
    cand_feat[base + r] = i;
  }
  if (!linear) proj_sync<kOneWave>();
  for (int k = tid; k < stride; k += nthreads) {
    if (k < n_cand) {
      if (!linear) {
        int first = k;
        const uint16_t c = s_cell[k];
        while (first > 0 && s_cell[first - 1] == c) first--;
        cand_first[base + k] = base + first;
      }
    } else {
      reqs[base + k].level = -1;  // dead slot: search_prepare / search_points skip it
      if (prep) {
        prep[base + k].alive = 0;
        prep[base + k].slevel = -1;
      }
    }
  }
  const int nblk = stride / kWavesPerBlock;
  for (int b = tid; b < nblk; b += nthreads) {
    int cnt = n_cand - b * kWavesPerBlock;
    cnt = cnt < 0 ? 0 : (cnt > kWavesPerBlock ? kWavesPerBlock : cnt);
    blocks[j * nblk + b] = SearchBlock{base + b * kWavesPerBlock, cnt};
  }
  if (tid == 0) {
    ChainFrameDev c;
    c.cand_begin = base;
    c.cand_end = base + n_cand;
    c.max_matches = jb.max_matches;
    c.rand_begin = j * max_its;
    c.obs_begin = j * mm;
    c.pad_ = 0;
#pragma unroll
    for (int q = 0; q < 7; q++) c.pose[q] = s_pose[q];
    c.pad2_ = 0.0;
    chain[j] = c;
  }
}

// dynamic LDS of track_commit_kernel for `stride` candidate slots and at most `mm` matches — s_before [stride + 1] 16-bit at 0 |
// s_found [stride] bytes | 64 spare | (8-byte aligned) s_depth [mm] doubles: byte offsets of the parts and the total
struct CommitLds {
  size_t found, depth, bytes;
  __host__ __device__ CommitLds(size_t stride, size_t mm) : found(2 * (stride + 1)), depth((found + stride + 64 + 7) / 8 * 8), bytes(depth + 8 * mm) {}
};

// second half of SelectPoints as bookkeeping (feature_align.cc:105-149), RemoveOutliers (:245-256), the new feature list
__global__ __launch_bounds__(256) void track_commit_kernel(const TrackJobDev *__restrict__ jobs, TrackPoint *__restrict__ points,
                                                           const TrackFeat *__restrict__ feats0_c, const TrackFeat *__restrict__ feats1_c,
                                                           TrackFeat *__restrict__ feats0, TrackFeat *__restrict__ feats1, int np, int nf, int stride,
                                                           int mm, const ChainFrameDev *__restrict__ chain, const int32_t *__restrict__ cand_first,
                                                           const int32_t *__restrict__ cand_feat, const sdvl_search_res *__restrict__ res,
                                                           const sdvl_pose_result *__restrict__ pres, const int32_t *__restrict__ lists,
                                                           const sdvl_align_result *__restrict__ ares, Cam cam, int max_failed,
                                                           SearchFramePose *__restrict__ registry, sdvl_track_result *__restrict__ h_results,
                                                           sdvl_track_feature_out *__restrict__ h_feats, sdvl_track_point_stat *__restrict__ h_stats) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  const CommitLds lds(stride, mm);
  uint16_t *s_before = reinterpret_cast<uint16_t *>(s_dyn);  // [stride + 1] matches selected among the candidates before k
  uint8_t *s_found = s_dyn + lds.found;                      // [stride]
  double *s_depth = reinterpret_cast<double *>(s_dyn + lds.depth);  // [mm] depths of the new frame's points
  __shared__ int s_wave[4];
  __shared__ int s_attempts, s_deleted, s_lk, s_npoints;
  __shared__ double s_median;
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TrackJobDev &jb = jobs[j];
  const ChainFrameDev &fr = chain[j];
  const int base = fr.cand_begin, n = fr.cand_end - fr.cand_begin;
  const TrackFeat *F = (jb.feat_buf ? feats1_c : feats0_c) + static_cast<size_t>(jb.tracker) * nf;
  TrackFeat *N = (jb.feat_buf ? feats0 : feats1) + static_cast<size_t>(jb.tracker) * nf;  // the OTHER buffer
  TrackPoint *P = points + static_cast<size_t>(jb.tracker) * np;
  if (tid == 0) { s_attempts = 0; s_deleted = 0; s_lk = 0; s_npoints = 0; }
  int lk = 0;
  for (int k = tid; k < n; k += 256) {
    const sdvl_search_res &r = res[base + k];
    s_found[k] = r.found != 0 ? 1 : 0;
    lk += r.lk_its;
  }
  __syncthreads();
  if (lk) atomicAdd(&s_lk, lk);
  // a cell's first found candidate is selected; s_before[k] = selected candidates before k
  int running = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int k = c0 + tid;
    bool sel = false;
    if (k < n && s_found[k]) {
      sel = true;
      for (int q = cand_first[base + k] - base; q < k; q++)
        if (s_found[q]) { sel = false; break; }
    }
    const unsigned long long m = __ballot(sel);
    const int below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
    __syncthreads();  // s_wave of the previous round has been read
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int b = running;
    for (int w = 0; w < wave; w++) b += s_wave[w];
    if (k < n) s_before[k] = static_cast<uint16_t>(b + below);
    running += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  }
  __syncthreads();
  const int matches = running < jb.max_matches ? running : jb.max_matches;
  // what the sequential loop does with candidate k: its cell is visited while fewer than max_matches matches exist; inside
  // the cell the candidates are tried until the first hit
  for (int k = tid; k < n; k += 256) {
    const int c0 = cand_first[base + k] - base;
    const bool visited = s_before[c0] < jb.max_matches;
    const bool tried = visited && s_before[k] == s_before[c0];
    if (!tried) continue;
    atomicAdd(&s_attempts, 1);
    const int fi = cand_feat[base + k];
    const int pt = F[fi].point;
    TrackPoint &p = P[pt];
    if (s_found[k]) {
      const sdvl_search_res &r = res[base + k];
      p.score += 1;      // Point::Promote
      p.n_failed = 0;
      p.status = (p.status & kKeepBits) | kFound;
      TrackFeat nf_;
      nf_.px[0] = r.px[0]; nf_.px[1] = r.px[1];
      const V3 v = cam_unproject(cam, {r.px[0], r.px[1]});  // Feature::Feature, feature.cc:28-35
      nf_.bearing[0] = v.x; nf_.bearing[1] = v.y; nf_.bearing[2] = v.z;
      nf_.level = r.level;
      nf_.point = pt;
      N[s_before[k]] = nf_;
    } else {
      p.n_failed += 1;   // Point::Unpromote; beyond MaxFailed the map deletes the point (feature_align.cc:141-142)
      int st = kNotFound;
      if (p.n_failed > max_failed && !(p.status & kDeleted)) {
        st |= kDeleted | (p.status & kTrash);
        atomicAdd(&s_deleted, 1);
      } else {
        st |= p.status & kKeepBits;
      }
      p.status = st;
    }
  }
  __syncthreads();
  // RemoveOutliers, feature_align.cc:245-256: the pose stage's outlier list indexes the matches
  const sdvl_pose_result pr = pres[j];
  const int32_t *lst = lists + fr.obs_begin;
  for (int q = tid; q < pr.n_outliers; q += 256) {
    const int r = lst[pr.n_inliers + q];
    const int pt = N[r].point;
    if (pt >= 0) {
      N[r].point = -1;
      P[pt].status = (P[pt].status & kKeepBits) | kNotFound;
    }
  }
  __syncthreads();
  int kept = 0;
  const Rigid final_pose = se3_from7(pr.pose);
  for (int r = tid; r < matches; r += 256) {
    const TrackFeat f = N[r];
    sdvl_track_feature_out o;
    o.px[0] = f.px[0]; o.px[1] = f.px[1];
    o.level = f.level;
    o.point = f.point;
    h_feats[static_cast<size_t>(j) * nf + r] = o;
    kept += f.point >= 0 ? 1 : 0;
    // Frame::GetSceneDepth, frame.cc:70-92: GetRelativePos(point position)(2) of every feature that has a point
    double z = __builtin_nan("");  // no point: compares false with everything below
    if (f.point >= 0) z = se3_apply(final_pose, {P[f.point].P[0], P[f.point].P[1], P[f.point].P[2]}).z;
    s_depth[r] = z;
  }
  if (kept) atomicAdd(&s_npoints, kept);
  if (tid == 0) s_median = 0.0;
  __syncthreads();
  {
    // GetMedianVector (extra/utils.cc:215-220): nth_element at floor(n / 2) = the value of sorted rank n / 2; a value v sits
    // there when fewer than or exactly n / 2 values are smaller and more than n / 2 are smaller or equal
    const int n_pts = s_npoints, mid = n_pts / 2;
    for (int r = tid; r < matches; r += 256) {
      const double v = s_depth[r];
      if (v != v) continue;
      int less = 0, leq = 0;
      for (int q = 0; q < matches; q++) {
        const double u = s_depth[q];
        less += u < v ? 1 : 0;
        leq += u <= v ? 1 : 0;
      }
      if (less <= mid && mid < leq) s_median = v;  // every writer holds the same value
    }
  }
  for (int q = tid; q < jb.n_points; q += 256) {
    TrackPoint &p = P[q];
    // a point the mapper deleted during the previous frame's update dies now: Map::DeletePoint only queues it, the queue is
    // emptied after the next frame has been tracked (sdvl.cc:127) — this frame still saw it
    if (p.status & kTrash) p.status = (p.status & ~kTrash) | kDeleted;
    sdvl_track_point_stat s;
    s.score = p.score; s.n_failed = p.n_failed; s.last_frame = p.last_frame; s.status = p.status;
    h_stats[static_cast<size_t>(j) * np + q] = s;
  }
  __syncthreads();
  if (tid == 0) {
    sdvl_track_result out;
#pragma unroll
    for (int q = 0; q < 7; q++) out.pose[q] = pr.pose[q];
    out.align_error = ares[j].error;
    out.scene_depth = s_median;
    out.align_meas = ares[j].n_meas;
    out.align_iters = ares[j].iters_run;
    out.n_features = jb.n_feat;
    out.n_requests = n;
    out.matches = matches;
    out.attempts = s_attempts;
    out.n_draws = pr.n_draws;
    out.n_inliers = pr.n_inliers;
    out.n_outliers = pr.n_outliers;
    out.refined = pr.refined;
    out.n_points = s_npoints;
    out.n_deleted = s_deleted;
    out.lk_iters = s_lk;
    out.n_corners = jb.cur.n_ptr[0];  // the new frame's corner count (header written by the detection's pack kernel)
    out.status = 0;
    h_results[j] = out;
#pragma unroll
    for (int q = 0; q < 7; q++) registry[jb.cur_id].pose[q] = pr.pose[q];  // the frame's final pose, for when it becomes a reference
  }
}

}  // namespace

struct sdvl_track_set {
  sdvl_ctx *ctx;
  int n, np, nf, cells, mm, max_its;
  // tables
  TrackPoint *d_points = nullptr;
  TrackFeat *d_feats[2] = {nullptr, nullptr};
  // per-step scratch, all sized for n jobs: parts of one allocation (cut up in sdvl_track_create)
  uint8_t *d_scratch = nullptr;
  sdvl_part<TrackJobDev> djobs;
  sdvl_part<uint16_t> cell_rank;
  sdvl_part<sdvl_align_result> ares;
  sdvl_part<SearchReqDev> reqs;
  sdvl_part<SearchPrep> prep;
  sdvl_part<sdvl_search_res> res;
  sdvl_part<double> reqpt;
  sdvl_part<int32_t> rand, cfirst, cfeat, lists, nobs;
  sdvl_part<SearchBlock> blocks;
  sdvl_part<ChainFrameDev> chain;
  sdvl_part<PoseJobDev> pjobs;
  sdvl_part<sdvl_pose_obs> obs;
  sdvl_part<uint8_t> hyp;
  sdvl_part<sdvl_pose_result> pres;
  // pinned host mirrors, written by track_commit
  uint8_t *h_pinned = nullptr;
  sdvl_track_result *h_results;
  sdvl_track_feature_out *h_feats;
  sdvl_track_point_stat *h_stats;
  // host view of the tables
  std::vector<int> n_points;
  std::vector<int> n_feat[2];
  // the step in flight
  std::vector<sdvl_track_job> jobs;
  int stride = 0;
  int phase = 0;  // 0 idle, 1 aligned, 2 searched
  uint32_t ticket = 0;
  sdvl_camera cam;
  sdvl_track_params prm;
};

extern "C" {

int sdvl_track_create(sdvl_ctx *ctx, int n, int max_points, int max_features, int grid_cells, int max_matches, int max_ransac_its,
                      sdvl_track_set **out) {
  if (!ctx || !out) return SDVL_ERR_INVALID;
  *out = nullptr;
  SDVL_REQUIRE(ctx, n >= 1 && n <= 65536, "tracker count out of range");
  SDVL_REQUIRE(ctx, max_points >= 1 && max_points < SDVL_TRACK_DUPLICATE && max_features >= 4 && max_features <= 4096, "table capacities out of range (features <= 4096)");
  SDVL_REQUIRE(ctx, grid_cells >= 1 && grid_cells <= 65535, "grid too large");
  SDVL_REQUIRE(ctx, max_matches >= 1 && max_matches <= 1024 && max_matches <= max_features, "max_matches outside the device pose stage's range (1024)");
  SDVL_REQUIRE(ctx, max_ransac_its >= 1 && max_ransac_its <= 4096, "bad max_ransac_its");
  SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
  sdvl_track_set *s = new sdvl_track_set();
  s->ctx = ctx;
  s->n = n;
  s->np = max_points;
  s->nf = (max_features + 3) / 4 * 4;
  s->cells = grid_cells;
  s->mm = max_matches;
  s->max_its = max_ransac_its;
  const size_t N = static_cast<size_t>(n), NF = N * s->nf;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->d_points), sizeof(TrackPoint) * N * s->np);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_feats[0]), sizeof(TrackFeat) * NF);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_feats[1]), sizeof(TrackFeat) * NF);
  sdvl_layout L;
  s->djobs = L.take<TrackJobDev>(N);  // jobs | cell ranks | rand values lead: sdvl_track_align pushes them as one block
  s->cell_rank = L.take<uint16_t>(N * s->cells);
  s->rand = L.take<int32_t>(N * s->max_its);
  s->ares = L.take<sdvl_align_result>(N);
  s->reqs = L.take<SearchReqDev>(NF);
  s->prep = L.take<SearchPrep>(NF);
  s->res = L.take<sdvl_search_res>(NF);
  s->reqpt = L.take<double>(NF * 3);
  s->cfirst = L.take<int32_t>(NF);
  s->cfeat = L.take<int32_t>(NF);
  s->blocks = L.take<SearchBlock>(NF / kWavesPerBlock);
  s->chain = L.take<ChainFrameDev>(N);
  // job and hypothesis records lie between the separate launches of a set of <= 4 trackers; larger sets' pose stage is one launch
  const bool separate = sdvl_pose_separate_launches(n);
  s->pjobs = L.take<PoseJobDev>(separate ? N : 0);
  s->obs = L.take<sdvl_pose_obs>(N * s->mm);
  s->hyp = L.take<uint8_t>(separate ? sdvl_pose_hyp_bytes() * N * s->max_its : 0);
  s->pres = L.take<sdvl_pose_result>(N);
  s->lists = L.take<int32_t>(N * s->mm);
  s->nobs = L.take<int32_t>(N);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_scratch), L.bytes());
  if (e == hipSuccess) {
    sdvl_layout H;  // pinned mirrors
    const sdvl_part<sdvl_track_result> results = H.take<sdvl_track_result>(N);
    const sdvl_part<sdvl_track_feature_out> feats = H.take<sdvl_track_feature_out>(NF);
    const sdvl_part<sdvl_track_point_stat> stats = H.take<sdvl_track_point_stat>(N * s->np);
    e = hipHostMalloc(reinterpret_cast<void **>(&s->h_pinned), H.bytes(), hipHostMallocDefault);
    if (e == hipSuccess) {
      memset(s->h_pinned, 0, H.bytes());
      s->h_results = results.in(s->h_pinned);
      s->h_feats = feats.in(s->h_pinned);
      s->h_stats = stats.in(s->h_pinned);
    }
  }
  if (e != hipSuccess) {
    ctx->err = std::string("sdvl_track_create: ") + hipGetErrorString(e);
    sdvl_track_destroy(ctx, s);
    return SDVL_ERR_HIP;
  }
  s->n_points.assign(n, 0);
  s->n_feat[0].assign(n, 0);
  s->n_feat[1].assign(n, 0);
  *out = s;
  return SDVL_OK;
}

TrackPoint *sdvl_track_points_device(sdvl_track_set *set, int *max_points, int *n_trackers) {
  if (max_points) *max_points = set->np;
  if (n_trackers) *n_trackers = set->n;
  return set->d_points;
}

int sdvl_track_destroy(sdvl_ctx *ctx, sdvl_track_set *s) {
  if (!ctx || !s) return SDVL_ERR_INVALID;
  (void)sdvl_bind_device(ctx);
  (void)sdvl_stream_wait(ctx);
  if (s->d_points) (void)hipFree(s->d_points);
  if (s->d_feats[0]) (void)hipFree(s->d_feats[0]);
  if (s->d_feats[1]) (void)hipFree(s->d_feats[1]);
  if (s->d_scratch) (void)hipFree(s->d_scratch);
  if (s->h_pinned) (void)hipHostFree(s->h_pinned);
  delete s;
  return SDVL_OK;
}

int sdvl_frame_register(sdvl_ctx *ctx, const sdvl_frame *f, const double *pose7) { return sdvl_frames_register(ctx, 1, &f, pose7); }

// n frames in one push + one launch (a group of trackers registers ~10 reference frames per step when keyframes are created:
// one at a time that was two dispatches each on the step's critical path)
int sdvl_frames_register(sdvl_ctx *ctx, int n, const sdvl_frame *const *frames, const double *poses7) {
  if (!ctx || n < 0 || (n > 0 && (!frames || !poses7))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  for (int i = 0; i < n; i++)
    SDVL_REQUIRE(ctx, frames[i] && frames[i]->home == ctx && frames[i]->reg_id >= 0 && frames[i]->reg_id < ctx->registry_cap,
                 "frame was not created on this context");
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_stage_alloc(ctx, sizeof(RegisterRec) * static_cast<size_t>(n), &hs, &dsx);
  if (rc) return rc;
  RegisterRec *r = static_cast<RegisterRec *>(hs);
  for (int i = 0; i < n; i++) {
    fill_view(&r[i].e.f, frames[i]);
    memcpy(r[i].e.pose, poses7 + 7 * i, sizeof(double) * 7);
    r[i].e.pad_ = 0.0;
    r[i].id = frames[i]->reg_id;
    r[i].pad_ = 0;
  }
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, sizeof(RegisterRec) * static_cast<size_t>(n)));
  SDVL_LAUNCH(ctx, "registry_write", registry_write_kernel, dim3((n + 63) / 64), dim3(64), static_cast<const RegisterRec *>(dsx), n,
              static_cast<SearchFramePose *>(ctx->d_registry));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  return SDVL_OK;
}

// append == false: the tables of the trackers are replaced; true: the rows go behind the rows the tables hold (round 4: a keyframe of
// the plane-map configuration adds its ~60 seeded points and their features to the tables the step has just updated on the device,
// instead of the host rebuilding all ~250 rows from Feature / Point objects)
static int track_upload_rows(sdvl_ctx *ctx, sdvl_track_set *s, int n, const int32_t *trackers, const int32_t *feat_buf, const int32_t *n_points,
                             const sdvl_track_point *points, const int32_t *n_features, const sdvl_track_feature *features, bool append) {
  if (!ctx || !s || s->ctx != ctx || n < 0 || (n > 0 && (!trackers || !feat_buf || !n_points || !n_features))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, s->phase == 0, "sdvl_track_upload while a step is in flight");
  size_t tp = 0, tf = 0;
  for (int i = 0; i < n; i++) {
    SDVL_REQUIRE(ctx, trackers[i] >= 0 && trackers[i] < s->n && (feat_buf[i] == 0 || feat_buf[i] == 1), "bad tracker / buffer index");
    const int p0 = append ? s->n_points[trackers[i]] : 0, f0 = append ? s->n_feat[feat_buf[i]][trackers[i]] : 0;
    if (n_points[i] < 0 || p0 + n_points[i] > s->np || n_features[i] < 0 || f0 + n_features[i] > s->nf) {
      ctx->err = "table larger than the set's capacity";
      return SDVL_ERR_CAPACITY;
    }
    for (int j = 0; j < i; j++) SDVL_REQUIRE(ctx, trackers[j] != trackers[i], "a tracker is named twice in one upload");
    tp += n_points[i];
    tf += n_features[i];
  }
  SDVL_REQUIRE(ctx, (tp == 0 || points) && (tf == 0 || features), "null rows");
  sdvl_layout st;  // staging: records | point rows | feature rows
  const sdvl_part<UploadRec> st_recs = st.take<UploadRec>(n);
  const sdvl_part<TrackPoint> st_points = st.take<TrackPoint>(tp);
  const sdvl_part<TrackFeat> st_feats = st.take<TrackFeat>(tf);
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
  if (rc) return rc;
  UploadRec *recs = st_recs.in(hs);
  TrackPoint *hp = st_points.in(hs);
  size_t po = 0, fo = 0;
  for (int i = 0; i < n; i++) {
    const int p0 = append ? s->n_points[trackers[i]] : 0, f0 = append ? s->n_feat[feat_buf[i]][trackers[i]] : 0;
    recs[i] = UploadRec{trackers[i], feat_buf[i], n_points[i], n_features[i], static_cast<long long>(po), static_cast<long long>(fo), p0, f0, 0};
    for (int k = 0; k < n_points[i]; k++) {
      const sdvl_track_point &src = points[po + k];
      SDVL_REQUIRE(ctx, src.ref && src.ref->home == ctx && src.ref->reg_id >= 0, "a point's reference frame was not created on this context");
      SDVL_REQUIRE(ctx, src.level >= 0 && src.level < src.ref->v.levels, "feature level outside the reference pyramid");
      SDVL_REQUIRE(ctx, src.idepth == src.idepth && src.idepth != 0.0, "inverse depth must be finite and non-zero");
      TrackPoint &d = hp[po + k];
      memcpy(&d, &src, sizeof(TrackPoint));  // same layout except for the frame pointer
      d.ref = src.ref->reg_id;
      d.pad_ = 0;
    }
    for (int k = 0; k < n_features[i]; k++) {
      const int pt = features[fo + k].point;
      SDVL_REQUIRE(ctx, pt < 0 || (pt & kPointMask) < p0 + n_points[i], "feature names a point outside its tracker's table");
    }
    po += n_points[i];
    fo += n_features[i];
  }
  if (tf) memcpy(st_feats.in(hs), features, st_feats.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
  SDVL_LAUNCH(ctx, "track_upload", track_upload_kernel, dim3(n), dim3(256), st_recs.cin(dsx), st_points.cin(dsx), st_feats.cin(dsx), s->d_points,
              s->d_feats[0], s->d_feats[1], s->np, s->nf);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  // every record was valid and the rows are on their way: only now do the host-side counts follow (a failed call leaves them untouched)
  for (int i = 0; i < n; i++) {
    s->n_points[trackers[i]] = recs[i].point_dst + n_points[i];
    s->n_feat[feat_buf[i]][trackers[i]] = recs[i].feat_dst + n_features[i];
  }
  return SDVL_OK;
}

int sdvl_track_upload(sdvl_ctx *ctx, sdvl_track_set *s, int n, const int32_t *trackers, const int32_t *feat_buf, const int32_t *n_points,
                      const sdvl_track_point *points, const int32_t *n_features, const sdvl_track_feature *features) {
  return track_upload_rows(ctx, s, n, trackers, feat_buf, n_points, points, n_features, features, false);
}

int sdvl_track_append(sdvl_ctx *ctx, sdvl_track_set *s, int n, const int32_t *trackers, const int32_t *feat_buf, const int32_t *n_points,
                      const sdvl_track_point *points, const int32_t *n_features, const sdvl_track_feature *features) {
  return track_upload_rows(ctx, s, n, trackers, feat_buf, n_points, points, n_features, features, true);
}

int sdvl_track_align(sdvl_ctx *ctx, sdvl_track_set *s, int n_jobs, const sdvl_track_job *jobs, const uint16_t *cell_rank, const int32_t *rand_raw,
                     const sdvl_camera *cam, const sdvl_track_params *p) {
  if (!ctx || !s || s->ctx != ctx || n_jobs <= 0 || !jobs || !cell_rank || !rand_raw || !cam || !p) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, s->phase == 0, "sdvl_track_align while a step is in flight");
  SDVL_REQUIRE(ctx, n_jobs <= s->n, "more jobs than trackers");
  int rc = sdvl_check_pose_params(ctx, &p->pose, s->max_its);
  if (rc) return rc;
  SDVL_REQUIRE(ctx, p->cell_size >= 1 && p->patch_size >= 0 && p->max_failed >= 0, "bad track parameters");
  {
    const int gw = static_cast<int>(ceil(cam->width / p->cell_size)), gh = static_cast<int>(ceil(cam->height / p->cell_size));
    SDVL_REQUIRE(ctx, gw * gh == s->cells, "the set's grid does not match camera / cell size");
  }
  int max_nf = 0;
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_track_job &a = jobs[j];
    SDVL_REQUIRE(ctx, a.tracker >= 0 && a.tracker < s->n && (a.feat_buf == 0 || a.feat_buf == 1), "bad tracker / buffer index");
    SDVL_REQUIRE(ctx, a.last && a.cur && a.last->home == ctx && a.cur->home == ctx, "frames of a job must be created on the set's context");
    SDVL_REQUIRE(ctx, a.max_matches >= 0 && a.max_matches <= s->mm, "max_matches above the set's");
    for (int q = 0; q < j; q++) SDVL_REQUIRE(ctx, jobs[q].tracker != a.tracker, "a tracker appears twice in one step");
    const int nf = s->n_feat[a.feat_buf][a.tracker];
    if (nf > max_nf) max_nf = nf;
  }
  for (int k = 0; k < n_jobs * s->cells; k++) SDVL_REQUIRE(ctx, cell_rank[k] < s->cells, "cell rank out of range");
  for (int k = 0; k < n_jobs * s->max_its; k++) SDVL_REQUIRE(ctx, rand_raw[k] >= 0, "rand() values are non-negative");
  rc = sdvl_ensure_nits_table(ctx, p->pose.max_ransac_points, p->pose.max_ransac_its, s->mm);
  if (rc) return rc;
  s->stride = (max_nf + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock;
  if (s->stride < kWavesPerBlock) s->stride = kWavesPerBlock;
  s->cam = *cam;
  s->prm = *p;
  s->jobs.assign(jobs, jobs + n_jobs);
  // jobs | cell ranks | rand values: the staged block mirrors the head of the set's scratch (the three parts lead it), part for part
  // at the scratch's own offsets, so ONE push lands all of them — every push is a launch on the step's critical path
  const size_t rand_bytes = sizeof(int32_t) * static_cast<size_t>(n_jobs) * s->max_its;
  const size_t head_bytes = s->rand.off + rand_bytes;
  void *hs = nullptr, *dsx = nullptr;
  rc = sdvl_stage_alloc(ctx, head_bytes, &hs, &dsx);
  if (rc) return rc;
  TrackJobDev *hj = s->djobs.in(hs);
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_track_job &a = jobs[j];
    TrackJobDev &d = hj[j];
    fill_view(&d.cur, a.cur, /*bins_pending*/ true);
    d.tracker = a.tracker;
    d.feat_buf = a.feat_buf;
    d.cur_id = a.cur->reg_id;
    d.last_id = a.last->reg_id;
    d.frame_id = a.frame_id;
    d.max_matches = a.max_matches;
    d.n_feat = s->n_feat[a.feat_buf][a.tracker];
    d.n_points = s->n_points[a.tracker];
    memcpy(d.last_pose, a.last_pose, sizeof(double) * 7);
    d.pad_ = 0.0;
    SDVL_REQUIRE(ctx, a.last->width == a.cur->width && a.last->height == a.cur->height && a.last->v.levels == a.cur->v.levels,
                 "frame pair with different geometry");
    for (int l = 0; l < SDVL_MAX_LEVELS; l++) d.last_level[l] = l < a.last->v.levels ? a.last->v.level[l] : nullptr;
    memcpy(d.T0, a.T, sizeof(double) * 7);
    d.pad2_ = 0.0;
  }
  memcpy(s->cell_rank.in(hs), cell_rank, sizeof(uint16_t) * static_cast<size_t>(n_jobs) * s->cells);
  memcpy(s->rand.in(hs), rand_raw, rand_bytes);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, s->d_scratch, hs, head_bytes));
  // the alignment reads the tables itself (image_align_track_*): no feature records, no launch in between
  rc = sdvl_image_align_track_enqueue(ctx, n_jobs, s->djobs.cin(s->d_scratch), static_cast<const TrackPoint *>(s->d_points),
                                      static_cast<const TrackFeat *>(s->d_feats[0]), static_cast<const TrackFeat *>(s->d_feats[1]), s->np, s->nf, max_nf,
                                      jobs[0].cur->v.levels, cam, &p->align, s->ares.in(s->d_scratch), s->n);
  if (rc) return rc;
  s->phase = 1;
  return SDVL_OK;
}

int sdvl_track_search(sdvl_ctx *ctx, sdvl_track_set *s) {
  if (!ctx || !s || s->ctx != ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, s->phase == 1, "sdvl_track_search without sdvl_track_align");
  const int n_jobs = static_cast<int>(s->jobs.size());
  for (const sdvl_track_job &a : s->jobs) {
    SDVL_REQUIRE(ctx, !a.cur->hdr_stale, "current frame has a new image but no corners (detect or set corners first)");
    SDVL_REQUIRE(ctx, s->prm.search.max_fast_levels <= a.cur->v.levels, "max_fast_levels exceeds the pyramid depth");
  }
  const Cam c = cam_of(s->cam);
  const int stride = s->stride;
  uint8_t *const D = s->d_scratch;
  SearchFramePose *registry = static_cast<SearchFramePose *>(ctx->d_registry);
  {
    // sdvl_track_align named the current frames' corner bins before the detection that fills them was queued (fill_view): frames
    // whose corners were set by hand instead have none
    static const bool never = getenv("SDVL_TRACK_NO_BINS") != nullptr;  // A/B and test of this path: every view loses its bins
    bool any = false;
    for (const sdvl_track_job &a : s->jobs) any = any || (a.cur->bin_cells > 0 && (never || !a.cur->bins_valid));
    for (const sdvl_track_job &a : s->jobs) ctx->counters[(a.cur->bin_cells > 0 && !never && a.cur->bins_valid) ? 0 : 1]++;
    if (any) {
      void *hs = nullptr, *dsx = nullptr;
      const int rc_m = sdvl_stage_alloc(ctx, static_cast<size_t>(n_jobs), &hs, &dsx);
      if (rc_m) return rc_m;
      uint8_t *hm = static_cast<uint8_t *>(hs);
      for (int j = 0; j < n_jobs; j++) hm[j] = (s->jobs[j].cur->bin_cells > 0 && (never || !s->jobs[j].cur->bins_valid)) ? 1 : 0;
      SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, static_cast<size_t>(n_jobs)));
      hipLaunchKernelGGL(track_clear_bins_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, ctx->stream, s->djobs.in(D), static_cast<const uint8_t *>(dsx), n_jobs);
      SDVL_HIP_CHECK(ctx, hipGetLastError());
    }
  }
  // track_project's lanes run SearchPoint's scalar phase for the requests they assemble: no search_prepare launch in a tracked step.
  // (The chain as a HIP graph was measured in rounds 4 and 5 — 2.69 k against 2.96 k frames/s for a lone camera, nothing for a farm:
  //  launches are not the cost — and removed in round 6.)
  // (one-time set-up calls stay outside a capture)
  const size_t proj_lds = ProjLds(stride, s->cells).bytes;
  if (proj_lds > kProjLdsDefault) {  // track_project beyond the default dynamic LDS limit (strides beyond 2000: only the wide form): raise it once per device
    static std::atomic<unsigned long long> attr_devices{0};
    const int rc_a = sdvl_allow_dynamic_lds(ctx, reinterpret_cast<const void *>(track_project_kernel<false>), kProjLdsMax, &attr_devices);
    if (rc_a) return rc_a;
  }
  {
    // a lane per feature of last_frame: 256 lanes cover the ~190 features of the metric configuration, configuration C's ~850 take 512.
    // A farm's launches (sets of more than 32 trackers) are workgroups of ONE wave up to stride kProjOneWaveStride: among the other
    // streams' one-wave workgroups a workgroup is placed when ALL its waves find a slot on one CU at the same moment, and the kernel's
    // dispatch time in company is how long its workgroups wait to be placed.  (Round 6, with the quadratic count of smaller keys: 256 ->
    // 128 threads 2.0 -> 1.5 ms per step of 16 groups; 64 threads gained less, the count's loop got longer.  The histogram has no such
    // loop.  Round 7: the flagship's groups are above stride 256 in nine launches of ten, which took the 512-thread form; the one
    // wave serves them too — figures in profiles/r07/track_project_one_wave.)
    const bool one_wave = stride <= kProjOneWaveStride && s->n > 32;
    const int proj_threads = one_wave ? 64 : (stride <= 256 ? 256 : kProjThreads);
#define SDVL_TRACK_PROJECT(kernel)                                                                                                                  \
  SDVL_LAUNCH_LDS(ctx, "track_project", kernel, dim3(n_jobs), dim3(proj_threads), proj_lds, s->djobs.cin(D), s->d_points,                          \
                  static_cast<const TrackFeat *>(s->d_feats[0]), static_cast<const TrackFeat *>(s->d_feats[1]), s->np, s->nf, stride, s->mm,        \
                  s->max_its, s->ares.cin(D), s->cell_rank.cin(D), s->cells, c, s->prm.cell_size, s->prm.patch_size, registry, s->reqs.in(D),      \
                  s->reqpt.in(D), s->cfirst.in(D), s->cfeat.in(D), s->blocks.in(D), s->chain.in(D), s->prm.search, s->prep.in(D))
    if (one_wave) SDVL_TRACK_PROJECT(track_project_kernel<true>);
    else SDVL_TRACK_PROJECT(track_project_kernel<false>);
#undef SDVL_TRACK_PROJECT
    SDVL_HIP_CHECK(ctx, hipGetLastError());
  }
  int rc = sdvl_search_launch_device(ctx, n_jobs * stride, s->reqs.in(D), registry, s->blocks.in(D), n_jobs * (stride / kWavesPerBlock), &s->cam,
                                     &s->prm.search, s->prep.in(D), s->res.in(D), nullptr, /*prepared*/ true);
  if (rc) return rc;
  // match ranks are not needed separately: track_commit derives them again from the same flags
  const PoseChainIn chain = {s->chain.cin(D), nullptr, s->cfirst.cin(D), s->res.cin(D), s->reqpt.cin(D), c, s->nobs.in(D), nullptr};
  const bool separate = sdvl_pose_separate_launches(s->n);
  sdvl_pose_params pp = s->prm.pose;
  pp.pad_ = 1;  // raw rand() values: the kernel reduces them modulo the match count it finds
  rc = sdvl_pose_enqueue_device(ctx, n_jobs, &chain, separate ? s->pjobs.in(D) : nullptr, s->obs.in(D), s->rand.in(D), static_cast<const int32_t *>(ctx->d_nits),
                                &pp, separate ? s->hyp.in(D) : nullptr, s->pres.in(D), s->lists.in(D), s->mm, s->n);
  if (rc) return rc;
  SDVL_LAUNCH_LDS(ctx, "track_commit", track_commit_kernel, dim3(n_jobs), dim3(256), CommitLds(stride, s->mm).bytes, s->djobs.cin(D), s->d_points,
                  static_cast<const TrackFeat *>(s->d_feats[0]), static_cast<const TrackFeat *>(s->d_feats[1]), s->d_feats[0], s->d_feats[1], s->np,
                  s->nf, stride, s->mm, s->chain.cin(D), s->cfirst.cin(D), s->cfeat.cin(D), s->res.cin(D), s->pres.cin(D), s->lists.cin(D),
                  s->ares.cin(D), c, s->prm.max_failed, registry, s->h_results, s->h_feats, s->h_stats);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, sdvl_mark_record(ctx, SDVL_MARK_CHAIN, &s->ticket));
  s->phase = 2;
  return SDVL_OK;
}

int sdvl_track_collect(sdvl_ctx *ctx, sdvl_track_set *s, int n_jobs, sdvl_track_result *results) {
  if (!ctx || !s || s->ctx != ctx || !results) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, s->phase == 2 && n_jobs == static_cast<int>(s->jobs.size()), "sdvl_track_collect without a matching sdvl_track_search");
  SDVL_HIP_CHECK(ctx, sdvl_mark_wait(ctx, SDVL_MARK_CHAIN, s->ticket));
  s->phase = 0;
  memcpy(results, s->h_results, sizeof(sdvl_track_result) * n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_track_job &a = s->jobs[j];
    s->n_feat[1 - a.feat_buf][a.tracker] = results[j].matches;
    if (results[j].n_corners >= 0) a.cur->v.n_corners = results[j].n_corners;  // the count rode along: no round trip to ask for it
  }
  ctx->wait_gen++;  // everything queued before the step's mark has completed (the detection's corner counts included)
  return SDVL_OK;
}

const sdvl_track_feature_out *sdvl_track_features(const sdvl_track_set *s, int job) {
  return (s && job >= 0 && job < s->n) ? s->h_feats + static_cast<size_t>(job) * s->nf : nullptr;
}

const sdvl_track_point_stat *sdvl_track_stats(const sdvl_track_set *s, int job) {
  return (s && job >= 0 && job < s->n) ? s->h_stats + static_cast<size_t>(job) * s->np : nullptr;
}

int sdvl_track_read_order(sdvl_ctx *ctx, const sdvl_track_set *s, int n_jobs, int capacity, int32_t *stride, int32_t *cand_first,
                          int32_t *cand_feat, int32_t *req_level, double *req_px, double *req_px0, int32_t *block_first, int32_t *block_count) {
  if (!ctx || !s || s->ctx != ctx || !stride || !cand_first || !cand_feat || !req_level || !req_px || !req_px0 || !block_first || !block_count)
    return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, s->phase == 0 && n_jobs >= 1 && n_jobs == static_cast<int>(s->jobs.size()), "sdvl_track_read_order without a collected step");
  const size_t slots = static_cast<size_t>(n_jobs) * s->stride;
  SDVL_REQUIRE(ctx, static_cast<size_t>(capacity) >= slots, "sdvl_track_read_order: arrays shorter than the step's slots");
  SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
  const uint8_t *D = s->d_scratch;
  std::vector<SearchReqDev> reqs(slots);
  std::vector<SearchBlock> blocks(slots / kWavesPerBlock);
  SDVL_HIP_CHECK(ctx, hipMemcpy(cand_first, s->cfirst.cin(D), sizeof(int32_t) * slots, hipMemcpyDeviceToHost));
  SDVL_HIP_CHECK(ctx, hipMemcpy(cand_feat, s->cfeat.cin(D), sizeof(int32_t) * slots, hipMemcpyDeviceToHost));
  SDVL_HIP_CHECK(ctx, hipMemcpy(reqs.data(), s->reqs.cin(D), sizeof(SearchReqDev) * slots, hipMemcpyDeviceToHost));
  SDVL_HIP_CHECK(ctx, hipMemcpy(blocks.data(), s->blocks.cin(D), sizeof(SearchBlock) * blocks.size(), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < slots; k++) {
    req_level[k] = reqs[k].level;
    req_px[2 * k] = reqs[k].px[0]; req_px[2 * k + 1] = reqs[k].px[1];
    req_px0[2 * k] = reqs[k].px0[0]; req_px0[2 * k + 1] = reqs[k].px0[1];
  }
  for (size_t b = 0; b < blocks.size(); b++) {
    block_first[b] = blocks[b].first;
    block_count[b] = blocks[b].count;
  }
  *stride = s->stride;
  return SDVL_OK;
}

}  // extern "C"
