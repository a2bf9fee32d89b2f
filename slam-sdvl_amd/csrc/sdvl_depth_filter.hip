// sdvl_depth_filter.hip — the mapper's depth filter: the body of Map::UpdateCandidates' loop behind SearchPoint (map.cc:454-497), one
// lane per request, for a search that has just run (sdvl_search_run_filter, sdvl_search_points_filter) or on search results the caller
// states (sdvl_depth_filter), and the same for a depth camera (the *_measured entries).  The arithmetic is sdvl_depth_filter.h's, shared
// with the host path; the search itself is sdvl_search.hip's.  A stereo rig has the same two entries (the *_stereo entries): the depth
// at the found pixel is the matcher's (stereo_lookup, sdvl_stereo.hip: one wave per request), launched between the search and the filter,
// whose third form reads what it left.  The host side is two bodies, searched and stated, over the three sources of depth.  Compiled with
// -ffp-contract=off.
#include "sdvl_internal.h"
#include "sdvl_math.h"
#include "sdvl_search_types.h"
#include "sdvl_stereo_device.h"
#include "sdvl_depth_filter.h"

namespace {

using namespace sdvl;

// the depth side of a measured call: the lookup's lens and rule, the noise model, the size of the depth images
struct DepthMeasure {
  sdvl_depth::DepthLens lens;
  sdvl_depth::DepthRule rule;
  double noise_abs, noise_quad;
  int32_t width, height;
};
// what the measured kernel takes besides the plain one's arguments.  jobs: the depth images; req_job: the job of every request (-1: none)
struct DepthMeasureArgs {
  const sdvl_depth::DepthJobDev *jobs;
  const int32_t *req_job;
  DepthMeasure dm;
  uint8_t *status, *status_host;  // the lookup's status per request, 255 for a request that made none
};

// the stereo side of a measured call: what stereo_lookup left per request (z, and the status: 255 for a request it looked nothing up
// for) and the noise model, tau = noise_quad z^2 with noise_quad = disparity_sigma / (fx baseline)
struct StereoMeasureArgs {
  const double *z;
  const uint8_t *status;
  double noise_quad;
  uint8_t *status_host;
};

enum FilterForm { kTriangulated = 0, kMeasured = 1, kStereo = 2 };

// the point's row in the tracking tables receives what the tracker reads of it
__device__ __forceinline__ void patch_row(TrackPoint *row, const sdvl_depth_out &o) {
  const int what = o.outcome & 0xFF;
  if (what == SDVL_DEPTH_NOT_FOUND) {
    row->n_failed = o.n_failed;
    if (o.outcome & SDVL_DEPTH_DELETED) row->status |= kTrash;
  } else if (what != SDVL_DEPTH_SKIPPED) {
    row->P[0] = o.position[0]; row->P[1] = o.position[1]; row->P[2] = o.position[2];
    if (what != SDVL_DEPTH_FIXED_STALE) {
      row->idepth = o.rho;
      row->idepth_std = sqrt(o.sigma2);  // Point::GetStd
      row->n_failed = 0;
    }
    if (what != SDVL_DEPTH_UPDATED) row->fixed = 1;
  }
}

// One lane per request, no LDS, no atomics.  kMeasured: a hit whose request names a depth image of its CURRENT frame looks the depth
// up at the found pixel by depth_seed's rule (depth_lookup, stride 1 << the found level); status OK: the measured update.  Any other
// status, or no image: the triangulated update, the same call of depth_filter_item with `measured` false and so the same bits.
// kStereo: the same with the depth and status that stereo_lookup left in HBM (m: a StereoMeasureArgs), noise_abs exactly 0.
template <int kForm, typename Measure = DepthMeasureArgs>
__device__ __forceinline__ void depth_filter_lane(const SearchReqDev *__restrict__ reqs, const SearchFramePose *__restrict__ table,
                                                  const sdvl_search_res *__restrict__ res, const sdvl_depth_state *__restrict__ state, int n,
                                                  const Cam &cam, const sdvl_depth_params &fp, TrackPoint *__restrict__ rows, int n_rows,
                                                  sdvl_depth_out *__restrict__ out, sdvl_depth_out *__restrict__ out_host,
                                                  const Measure *m = nullptr) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= n) return;
  const SearchReqDev &rq = reqs[i];
  const sdvl_depth_state st = state[i];
  const sdvl_search_res r = res[i];
  sdvl_depth_out o;
  if constexpr (kForm == kStereo) {
    const int status = m->status[i];
    o = depth_filter_item(table[rq.cur].pose, table[rq.ref].pose, rq.bearing, r.found != 0, r.px, st, cam, fp, status == SDVL_STEREO_OK, m->z[i], 0.0,
                          m->noise_quad);
    if (m->status_host) m->status_host[i] = static_cast<uint8_t>(status);
  } else if constexpr (kForm == kMeasured) {
    int status = 255;
    double zc = 0.0;
    const int jb = m->req_job[i];
    if (r.found && jb >= 0) {
      const int l = r.level < 0 ? 0 : (r.level >= SDVL_MAX_LEVELS ? SDVL_MAX_LEVELS - 1 : r.level);
      status = sdvl_depth::depth_lookup(m->jobs[jb], r.px[0], r.px[1], 1 << l, m->dm.width, m->dm.height, m->dm.lens, m->dm.rule, &zc);
    }
    o = depth_filter_item(table[rq.cur].pose, table[rq.ref].pose, rq.bearing, r.found != 0, r.px, st, cam, fp, status == SDVL_DEPTH_SEED_OK, zc,
                          m->dm.noise_abs, m->dm.noise_quad);
    m->status[i] = static_cast<uint8_t>(status);
    if (m->status_host) m->status_host[i] = static_cast<uint8_t>(status);
  } else {
    o = depth_filter_item(table[rq.cur].pose, table[rq.ref].pose, rq.bearing, r.found != 0, r.px, st, cam, fp);
  }
  if (rows && st.track_row >= 0 && st.track_row < n_rows) patch_row(rows + st.track_row, o);
  out[i] = o;
  if (out_host) out_host[i] = o;
}

__global__ __launch_bounds__(128) void depth_filter_kernel(const SearchReqDev *__restrict__ reqs, const SearchFramePose *__restrict__ table,
                                                           const sdvl_search_res *__restrict__ res, const sdvl_depth_state *__restrict__ state,
                                                           int n, Cam cam, sdvl_depth_params fp, TrackPoint *__restrict__ rows, int n_rows,
                                                           sdvl_depth_out *__restrict__ out, sdvl_depth_out *__restrict__ out_host) {
  depth_filter_lane<kTriangulated>(reqs, table, res, state, n, cam, fp, rows, n_rows, out, out_host);
}

__global__ __launch_bounds__(128) void depth_filter_measured_kernel(const SearchReqDev *__restrict__ reqs, const SearchFramePose *__restrict__ table,
                                                                    const sdvl_search_res *__restrict__ res, const sdvl_depth_state *__restrict__ state,
                                                                    int n, Cam cam, sdvl_depth_params fp, TrackPoint *__restrict__ rows, int n_rows,
                                                                    sdvl_depth_out *__restrict__ out, sdvl_depth_out *__restrict__ out_host,
                                                                    DepthMeasureArgs m) {
  depth_filter_lane<kMeasured>(reqs, table, res, state, n, cam, fp, rows, n_rows, out, out_host, &m);
}

__global__ __launch_bounds__(128) void depth_filter_stereo_kernel(const SearchReqDev *__restrict__ reqs, const SearchFramePose *__restrict__ table,
                                                                  const sdvl_search_res *__restrict__ res, const sdvl_depth_state *__restrict__ state,
                                                                  int n, Cam cam, sdvl_depth_params fp, TrackPoint *__restrict__ rows, int n_rows,
                                                                  sdvl_depth_out *__restrict__ out, sdvl_depth_out *__restrict__ out_host,
                                                                  StereoMeasureArgs m) {
  depth_filter_lane<kStereo, StereoMeasureArgs>(reqs, table, res, state, n, cam, fp, rows, n_rows, out, out_host, &m);
}

// ---- what every entry requires of the states; -> the rows the kernel may patch (none without a set)
int depth_filter_check(sdvl_ctx *ctx, int n, const sdvl_depth_state *state, sdvl_track_set *set, TrackPoint **rows_out, int *n_rows_out) {
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  if (set) {
    int np = 0, nt = 0;
    rows = sdvl_track_points_device(set, &np, &nt);
    n_rows = np * nt;
  }
  for (int i = 0; i < n; i++) {
    SDVL_REQUIRE(ctx, state[i].track_row >= -1 && (state[i].track_row < n_rows || !set), "depth filter: track_row outside the tables");
    SDVL_REQUIRE(ctx, state[i].sigma2 > 0.0 && state[i].z_range > 0.0, "depth filter: sigma2 and z_range must be positive");
  }
  *rows_out = rows;
  *n_rows_out = n_rows;
  return SDVL_OK;
}

// what the measured entries require of the depth side; -> the kernel's record
int depth_measure_check(sdvl_ctx *ctx, const char *who, int n, int n_jobs, const sdvl_depth_job *jobs, int width, int height, const sdvl_camera *cam,
                        const sdvl_distortion *dist, const sdvl_depth_measure_params *mp, DepthMeasure *dm) {
  const std::string w(who);
  SDVL_REQUIRE(ctx, n_jobs >= 0 && (n_jobs == 0 || jobs), w + ": bad job list");
  int rc = sdvl_depth_rule_of(ctx, who, mp ? &mp->rule : nullptr, &dm->rule);
  if (!rc) rc = sdvl_depth_jobs_check(ctx, who, n_jobs, jobs, width, height, n);
  if (rc) return rc;
  dm->noise_abs = SDVL_DEPTH_NOISE_ABS;
  dm->noise_quad = SDVL_DEPTH_NOISE_QUAD;
  if (mp) {
    SDVL_REQUIRE(ctx, mp->noise_abs >= 0.0 && mp->noise_quad >= 0.0, w + ": noise_abs and noise_quad must not be negative");
    if (mp->noise_abs != 0.0) dm->noise_abs = mp->noise_abs;
    if (mp->noise_quad != 0.0) dm->noise_quad = mp->noise_quad;
  }
  dm->lens = sdvl_depth_lens_of(cam, dist);
  dm->width = width;
  dm->height = height;
  return SDVL_OK;
}

// what the stereo entries require of the stereo side; -> the matcher's rule (its LDS sized for the coarsest level of the jobs' left
// frames: the levels of a search's hits are not known on the host when the launch is queued) and the noise
int stereo_measure_check(sdvl_ctx *ctx, const char *who, int n, int n_jobs, const sdvl_stereo_job *jobs, const sdvl_camera *cam,
                         const sdvl_stereo_measure_params *mp, sdvl_stereo::StereoRule *rule, size_t *lds_bytes, double *noise_quad) {
  const std::string w(who);
  SDVL_REQUIRE(ctx, n_jobs >= 0 && (n_jobs == 0 || jobs), w + ": bad job list");
  SDVL_REQUIRE(ctx, mp != nullptr, w + ": null parameters (the baseline has no default)");
  SDVL_REQUIRE(ctx, mp->disparity_sigma >= 0.0 && mp->disparity_sigma <= 1.79769313486231570815e308, w + ": disparity_sigma negative or not finite");
  int rc = sdvl_stereo_rule_of(ctx, who, cam, &mp->rule, rule);
  if (!rc) rc = sdvl_stereo_jobs_check(ctx, who, "request", n_jobs, jobs, n);
  if (rc) return rc;
  int max_level = 0;
  for (int j = 0; j < n_jobs; j++) max_level = jobs[j].left->v.levels - 1 > max_level ? jobs[j].left->v.levels - 1 : max_level;
  *noise_quad = (mp->disparity_sigma != 0.0 ? mp->disparity_sigma : SDVL_STEREO_DISPARITY_SIGMA) / rule->fb;
  return sdvl_stereo_lds(ctx, who, max_level, rule, lds_bytes);
}

// what the stated entries with a level per item require of it
int found_levels_check(sdvl_ctx *ctx, const char *who, int n, const int32_t *level) {
  for (int i = 0; i < n; i++)
    SDVL_REQUIRE(ctx, level[i] >= 0 && level[i] < SDVL_MAX_LEVELS, std::string(who) + ": found level outside 0 .. SDVL_MAX_LEVELS - 1");
  return SDVL_OK;
}

// ---- the three sources of the depth at a found pixel.  The six entries are two bodies (filter_searched, filter_stated) over a source,
// which states only what is its own: its entry's name for the messages (who), its check, the check of the levels a caller states, its
// parts of the result buffers (d: d_out, h: the pinned h_out, both behind the outcomes) and of the staging block (behind the body's
// own) with their fill, what it queues between the search results and the filter, its launch of the filter (head: the arguments the
// three kernels share) and what it copies out besides the outcomes.
struct Triangulated {
  int check(sdvl_ctx *, int, const sdvl_camera *) { return SDVL_OK; }
  int levels_check(sdvl_ctx *, int, const int32_t *, const int32_t *) const { return SDVL_OK; }
  void take_out(sdvl_layout &, sdvl_layout &, int) {}
  void take_stage(sdvl_layout &, int) {}
  int fill(sdvl_ctx *, void *, int) const { return SDVL_OK; }
  int enqueue(sdvl_ctx *, int, const void *, const sdvl_search_res *) const { return SDVL_OK; }
  template <typename... Head>
  void launch(sdvl_ctx *ctx, int n, const void *, Head... head) const {
    SDVL_LAUNCH(ctx, "depth_filter", depth_filter_kernel, dim3((n + 127) / 128), dim3(128), head...);
  }
  void collect(const sdvl_ctx *, int) const {}
};

// a registered depth image per job.  d and h: the status bytes (the kernel writes both); staged: jobs | the job of every request (-1: none)
struct FromDepthImage {
  const char *who;
  int n_jobs;
  const sdvl_depth_job *jobs;
  int width, height;
  const sdvl_distortion *dist;
  const sdvl_depth_measure_params *mp;
  uint8_t *out_status;
  DepthMeasure dm;
  sdvl_part<uint8_t> d_status, h_status;
  sdvl_part<sdvl_depth::DepthJobDev> st_jobs;
  sdvl_part<int32_t> st_req_job;
  int check(sdvl_ctx *ctx, int n, const sdvl_camera *cam) { return depth_measure_check(ctx, who, n, n_jobs, jobs, width, height, cam, dist, mp, &dm); }
  int levels_check(sdvl_ctx *ctx, int n, const int32_t *, const int32_t *level) const { return found_levels_check(ctx, who, n, level); }
  void take_out(sdvl_layout &d, sdvl_layout &h, int n) { d_status = d.take<uint8_t>(n), h_status = h.take<uint8_t>(n); }
  void take_stage(sdvl_layout &st, int n) { st_jobs = st.take<sdvl_depth::DepthJobDev>(n_jobs > 0 ? n_jobs : 1), st_req_job = st.take<int32_t>(n); }
  int fill(sdvl_ctx *ctx, void *hs, int n) const {
    const int rc = n_jobs > 0 ? sdvl_depth_jobs_resolve(ctx, n_jobs, jobs, width, height, st_jobs.in(hs)) : SDVL_OK;
    if (rc) return rc;
    sdvl_item_jobs_fill(n, n_jobs, jobs, st_req_job.in(hs));  // (ranges that overlap: the later job's)
    return SDVL_OK;
  }
  int enqueue(sdvl_ctx *, int, const void *, const sdvl_search_res *) const { return SDVL_OK; }
  template <typename... Head>
  void launch(sdvl_ctx *ctx, int n, const void *ds, Head... head) const {
    const DepthMeasureArgs m = {st_jobs.cin(ds), st_req_job.cin(ds), dm, d_status.in(ctx->d_out), h_status.in(ctx->h_out)};
    SDVL_LAUNCH(ctx, "depth_filter_measured", depth_filter_measured_kernel, dim3((n + 127) / 128), dim3(128), head..., m);
  }
  void collect(const sdvl_ctx *ctx, int n) const { memcpy(out_status, h_status.in(ctx->h_out), static_cast<size_t>(n)); }
};

// a rectified pair per job: stereo_lookup (sdvl_stereo.hip: one wave per request) over the search results where they lie, the filter's
// third form on what it left.  d: z | the status bytes, h: the status bytes (the filter writes them); staged: as FromDepthImage's
struct FromStereoPair {
  const char *who;
  int n_jobs;
  const sdvl_stereo_job *jobs;
  const sdvl_stereo_measure_params *mp;
  uint8_t *out_status;
  sdvl_stereo::StereoRule rule;
  size_t lds_bytes;
  double noise_quad;
  sdvl_part<double> d_z;
  sdvl_part<uint8_t> d_status, h_status;
  sdvl_part<sdvl_stereo::StereoJobDev> st_jobs;
  sdvl_part<int32_t> st_req_job;
  int check(sdvl_ctx *ctx, int n, const sdvl_camera *cam) { return stereo_measure_check(ctx, who, n, n_jobs, jobs, cam, mp, &rule, &lds_bytes, &noise_quad); }
  // the matcher reads the left frame's pyramid on a hit's level (a miss's level is not looked at)
  int levels_check(sdvl_ctx *ctx, int n, const int32_t *found, const int32_t *level) const {
    const int rc = found_levels_check(ctx, who, n, level);
    if (rc) return rc;
    for (int j = 0; j < n_jobs; j++)
      for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++)
        SDVL_REQUIRE(ctx, !found[i] || level[i] < jobs[j].left->v.levels, std::string(who) + ": a hit's level lies outside the left frame's pyramid");
    return SDVL_OK;
  }
  void take_out(sdvl_layout &d, sdvl_layout &h, int n) { d_z = d.take<double>(n), d_status = d.take<uint8_t>(n), h_status = h.take<uint8_t>(n); }
  void take_stage(sdvl_layout &st, int n) { st_jobs = st.take<sdvl_stereo::StereoJobDev>(n_jobs > 0 ? n_jobs : 1), st_req_job = st.take<int32_t>(n); }
  int fill(sdvl_ctx *ctx, void *hs, int n) const {
    SDVL_REQUIRE(ctx, !sdvl_item_jobs_fill(n, n_jobs, jobs, st_req_job.in(hs)), std::string(who) + ": request ranges overlap");
    return n_jobs > 0 ? sdvl_stereo_jobs_resolve(ctx, n_jobs, jobs, st_jobs.in(hs)) : sdvl_depth_pool_scope(ctx);
  }
  int enqueue(sdvl_ctx *ctx, int n, const void *ds, const sdvl_search_res *d_res) const {
    return sdvl_stereo_lookup_enqueue(ctx, n, st_jobs.cin(ds), d_res, st_req_job.cin(ds), rule, lds_bytes, d_z.in(ctx->d_out), d_status.in(ctx->d_out));
  }
  template <typename... Head>
  void launch(sdvl_ctx *ctx, int n, const void *, Head... head) const {
    const StereoMeasureArgs m = {d_z.cin(ctx->d_out), d_status.cin(ctx->d_out), noise_quad, h_status.in(ctx->h_out)};
    SDVL_LAUNCH(ctx, "depth_filter_stereo", depth_filter_stereo_kernel, dim3((n + 127) / 128), dim3(128), head..., m);
  }
  void collect(const sdvl_ctx *ctx, int n) const { memcpy(out_status, h_status.in(ctx->h_out), static_cast<size_t>(n)); }
};

// Search results the caller states, as the records a search leaves: requests | frame table (entry 2i: item i's current pose, 2i + 1:
// its reference pose) | search results | states.  Of a request the kernel reads the two slots and the bearing, of a table entry the
// pose, of a result `found`, `px` and (measured) `level`: everything else stays zero.  level may be null
struct StatedStage {
  sdvl_part<SearchReqDev> reqs;
  sdvl_part<SearchFramePose> tab;
  sdvl_part<sdvl_search_res> res;
  sdvl_part<sdvl_depth_state> state;
  StatedStage(sdvl_layout &st, int n)
      : reqs(st.take<SearchReqDev>(n)), tab(st.take<SearchFramePose>(2 * static_cast<size_t>(n))), res(st.take<sdvl_search_res>(n)),
        state(st.take<sdvl_depth_state>(n)) {}
  // hs: the staging block, zeroed
  void fill(void *hs, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found, const double *px,
            const int32_t *level, const sdvl_depth_state *states) const {
    SearchReqDev *hreq = reqs.in(hs);
    SearchFramePose *htab = tab.in(hs);
    sdvl_search_res *hres = res.in(hs);
    for (int i = 0; i < n; i++) {
      hreq[i].cur = 2 * i;
      hreq[i].ref = 2 * i + 1;
      memcpy(hreq[i].bearing, bearing + 3 * static_cast<size_t>(i), sizeof(double) * 3);
      memcpy(htab[2 * i].pose, cur_pose + 7 * static_cast<size_t>(i), sizeof(double) * 7);
      memcpy(htab[2 * i + 1].pose, ref_pose + 7 * static_cast<size_t>(i), sizeof(double) * 7);
      hres[i].found = found[i] ? 1 : 0;
      if (level) hres[i].level = level[i];
      hres[i].px[0] = px[2 * static_cast<size_t>(i)];
      hres[i].px[1] = px[2 * static_cast<size_t>(i) + 1];
    }
    memcpy(state.in(hs), states, state.bytes());
  }
};

// Behind the one push of a body's staging block ds: what the source queues first, its launch over records that lie in HBM, the wait, and
// the outcomes with what the source adds into the caller's arrays.  out / out_host: the outcomes' places in d_out and in the pinned
// h_out, which the kernel writes itself
struct FilterRecords {
  const SearchReqDev *reqs;
  const SearchFramePose *table;
  const sdvl_search_res *res;
  const sdvl_depth_state *state;
  sdvl_depth_out *out, *out_host;
};
template <typename Source>
int filter_launch_collect(sdvl_ctx *ctx, const Source &src, int n, const void *ds, const FilterRecords &r, const sdvl_camera *cam,
                          const sdvl_depth_params *fp, TrackPoint *rows, int n_rows, sdvl_depth_out *fout) {
  const int rc = src.enqueue(ctx, n, ds, r.res);
  if (rc) return rc;
  src.launch(ctx, n, ds, r.reqs, r.table, r.res, r.state, n, cam_of(*cam), *fp, rows, n_rows, r.out, r.out_host);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  memcpy(fout, r.out_host, sizeof(sdvl_depth_out) * static_cast<size_t>(n));
  src.collect(ctx, n);
  return SDVL_OK;
}

// search + depth filter (Map::UpdateCandidates, map.cc:402-498) over the batch the context holds: one submission, one wait.  d_out:
// the search's | the outcomes | the source's; h_out: the search results | the outcomes | the source's; staged: the states | the source's
template <typename Source>
int filter_searched(sdvl_ctx *ctx, Source &src, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                    const sdvl_depth_params *fp, sdvl_track_set *set, sdvl_search_res *out, sdvl_depth_out *fout) {
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (!rc) rc = src.check(ctx, n, cam);
  if (rc) return rc;
  SearchOut so(n);
  const sdvl_part<sdvl_depth_out> d_fout = so.d.take<sdvl_depth_out>(n), h_fout = so.h.take<sdvl_depth_out>(n);
  src.take_out(so.d, so.h, n);
  FilterRecords r = {};
  rc = sdvl_search_enqueue(ctx, n, cam, p, so, &r.reqs, &r.table);
  if (rc) return rc;
  sdvl_layout st;
  const sdvl_part<sdvl_depth_state> st_state = st.take<sdvl_depth_state>(n);
  src.take_stage(st, n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &ds);
  if (!rc) rc = src.fill(ctx, hs, n);
  if (rc) return rc;
  memcpy(st_state.in(hs), state, st_state.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  r.res = so.res.cin(ctx->d_out), r.state = st_state.cin(ds), r.out = d_fout.in(ctx->d_out), r.out_host = h_fout.in(ctx->h_out);
  rc = filter_launch_collect(ctx, src, n, ds, r, cam, fp, rows, n_rows, fout);
  if (rc) return rc;
  memcpy(out, so.h_res.in(ctx->h_out), so.h_res.bytes());
  return SDVL_OK;
}

// the depth filter alone, on search results the caller states (level: null where the source reads none).  d_out and h_out: the outcomes |
// the source's; staged: StatedStage | the source's, zeroed
template <typename Source>
int filter_stated(sdvl_ctx *ctx, Source &src, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                  const double *px, const int32_t *level, const sdvl_camera *cam, const sdvl_depth_state *state, const sdvl_depth_params *fp,
                  sdvl_track_set *set, sdvl_depth_out *fout) {
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (!rc) rc = src.check(ctx, n, cam);
  if (!rc) rc = src.levels_check(ctx, n, found, level);
  if (rc) return rc;
  sdvl_layout st, d, h;
  const StatedStage stated(st, n);
  src.take_stage(st, n);
  const sdvl_part<sdvl_depth_out> d_fout = d.take<sdvl_depth_out>(n), h_fout = h.take<sdvl_depth_out>(n);
  src.take_out(d, h, n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_reserve_out_stage(ctx, d.bytes() > h.bytes() ? d.bytes() : h.bytes(), st.bytes(), &hs, &ds);
  if (rc) return rc;
  memset(hs, 0, st.bytes());
  rc = src.fill(ctx, hs, n);
  if (rc) return rc;
  stated.fill(hs, n, cur_pose, ref_pose, bearing, found, px, level, state);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  const FilterRecords r = {stated.reqs.cin(ds), stated.tab.cin(ds), stated.res.cin(ds), stated.state.cin(ds), d_fout.in(ctx->d_out), h_fout.in(ctx->h_out)};
  return filter_launch_collect(ctx, src, n, ds, r, cam, fp, rows, n_rows, fout);
}

}  // namespace

extern "C" {

// ---- each entry: its null arguments, the empty call, its source, one of the two bodies
int sdvl_search_run_filter(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                           const sdvl_depth_params *fp, sdvl_track_set *set, sdvl_search_res *out, sdvl_depth_out *fout) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!state || !out || !fout))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  Triangulated src;
  return filter_searched(ctx, src, n, cam, p, state, fp, set, out, fout);
}

int sdvl_search_points_filter(sdvl_ctx *ctx, int n, const sdvl_search_req *reqs, const sdvl_camera *cam, const sdvl_search_params *p,
                              const sdvl_depth_state *state, const sdvl_depth_params *fp, sdvl_track_set *set, sdvl_search_res *out,
                              sdvl_depth_out *fout) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!reqs || !state || !out || !fout))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  const int rc = sdvl_search_pack_requests(ctx, n, reqs);
  if (rc) return rc;
  return sdvl_search_run_filter(ctx, n, cam, p, state, fp, set, out, fout);
}

int sdvl_depth_filter(sdvl_ctx *ctx, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                      const double *px, const sdvl_camera *cam, const sdvl_depth_state *state, const sdvl_depth_params *fp,
                      sdvl_track_set *set, sdvl_depth_out *fout) {
  if (!ctx || !cam || !fp || n < 0 || (n > 0 && (!cur_pose || !ref_pose || !bearing || !found || !px || !state || !fout))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  Triangulated src;
  return filter_stated(ctx, src, n, cur_pose, ref_pose, bearing, found, px, nullptr, cam, state, fp, set, fout);
}

// ---- the same two entries for a depth camera
int sdvl_search_run_filter_measured(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                                    const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_depth_job *jobs, int width, int height,
                                    const sdvl_distortion *dist, const sdvl_depth_measure_params *mp, sdvl_search_res *out, sdvl_depth_out *fout,
                                    uint8_t *out_status) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!state || !out || !fout || !out_status))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  FromDepthImage src = {"sdvl_search_run_filter_measured", n_jobs, jobs, width, height, dist, mp, out_status};
  return filter_searched(ctx, src, n, cam, p, state, fp, set, out, fout);
}

int sdvl_depth_filter_measured(sdvl_ctx *ctx, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                               const double *px, const int32_t *level, const sdvl_camera *cam, const sdvl_depth_state *state,
                               const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_depth_job *jobs, int width, int height,
                               const sdvl_distortion *dist, const sdvl_depth_measure_params *mp, sdvl_depth_out *fout, uint8_t *out_status) {
  if (!ctx || !cam || !fp || n < 0 || (n > 0 && (!cur_pose || !ref_pose || !bearing || !found || !px || !level || !state || !fout || !out_status)))
    return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  FromDepthImage src = {"sdvl_depth_filter_measured", n_jobs, jobs, width, height, dist, mp, out_status};
  return filter_stated(ctx, src, n, cur_pose, ref_pose, bearing, found, px, level, cam, state, fp, set, fout);
}

// ---- and for a stereo rig
int sdvl_search_run_filter_stereo(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                                  const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_stereo_job *jobs,
                                  const sdvl_stereo_measure_params *mp, sdvl_search_res *out, sdvl_depth_out *fout, uint8_t *out_status) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!state || !out || !fout || !out_status))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  FromStereoPair src = {"sdvl_search_run_filter_stereo", n_jobs, jobs, mp, out_status};
  return filter_searched(ctx, src, n, cam, p, state, fp, set, out, fout);
}

int sdvl_depth_filter_stereo(sdvl_ctx *ctx, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                             const double *px, const int32_t *level, const sdvl_camera *cam, const sdvl_depth_state *state,
                             const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_stereo_job *jobs,
                             const sdvl_stereo_measure_params *mp, sdvl_depth_out *fout, uint8_t *out_status) {
  if (!ctx || !cam || !fp || n < 0 || (n > 0 && (!cur_pose || !ref_pose || !bearing || !found || !px || !level || !state || !fout || !out_status)))
    return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  FromStereoPair src = {"sdvl_depth_filter_stereo", n_jobs, jobs, mp, out_status};
  return filter_stated(ctx, src, n, cur_pose, ref_pose, bearing, found, px, level, cam, state, fp, set, fout);
}

}  // extern "C"
