// sdvl_depth_filter.hip — the mapper's depth filter: the body of Map::UpdateCandidates' loop behind SearchPoint (map.cc:454-497), one
// lane per request, for a search that has just run (sdvl_search_run_filter, sdvl_search_points_filter) or on search results the caller
// states (sdvl_depth_filter), and the same for a depth camera (the *_measured entries).  The arithmetic is sdvl_depth_filter.h's, shared
// with the host path; the search itself is sdvl_search.hip's.  A stereo rig has the same two entries (the *_stereo entries): the depth
// at the found pixel is the matcher's (stereo_lookup, sdvl_stereo.hip: one wave per request), launched between the search and the filter,
// whose third form reads what it left.  Compiled with -ffp-contract=off.
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

// ---- what the seven entries share
// what every entry requires of the states; -> the rows the kernel may patch (none without a set)
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

// jobs | the job of every request (-1: none) as one staged record
struct StereoMeasureStage {
  sdvl_part<sdvl_stereo::StereoJobDev> jobs;
  sdvl_part<int32_t> req_job;
  StereoMeasureStage(sdvl_layout &st, int n, int n_jobs) : jobs(st.take<sdvl_stereo::StereoJobDev>(n_jobs > 0 ? n_jobs : 1)), req_job(st.take<int32_t>(n)) {}
  int fill(sdvl_ctx *ctx, const char *who, void *hs, int n, int n_jobs, const sdvl_stereo_job *in) const {
    SDVL_REQUIRE(ctx, !sdvl_item_jobs_fill(n, n_jobs, in, req_job.in(hs)), std::string(who) + ": request ranges overlap");
    return n_jobs > 0 ? sdvl_stereo_jobs_resolve(ctx, n_jobs, in, jobs.in(hs)) : sdvl_depth_pool_scope(ctx);
  }
};

// jobs | the job of every request (-1: none) as one staged record
struct DepthMeasureStage {
  sdvl_part<sdvl_depth::DepthJobDev> jobs;
  sdvl_part<int32_t> req_job;
  DepthMeasureStage(sdvl_layout &st, int n, int n_jobs) : jobs(st.take<sdvl_depth::DepthJobDev>(n_jobs > 0 ? n_jobs : 1)), req_job(st.take<int32_t>(n)) {}
  int fill(sdvl_ctx *ctx, void *hs, int n, int n_jobs, const sdvl_depth_job *in, int width, int height) const {
    const int rc = n_jobs > 0 ? sdvl_depth_jobs_resolve(ctx, n_jobs, in, width, height, jobs.in(hs)) : SDVL_OK;
    if (rc) return rc;
    sdvl_item_jobs_fill(n, n_jobs, in, req_job.in(hs));  // (ranges that overlap: the later job's)
    return SDVL_OK;
  }
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

// One launch over records that lie in HBM, the wait, and the outcomes (with a measured part m: and the status bytes) into the caller's
// arrays.  d_fout / h_fout, m->status / m->status_host: their places in d_out and in the pinned h_out, which the kernel writes itself
int filter_launch_collect(sdvl_ctx *ctx, int n, const SearchReqDev *d_reqs, const SearchFramePose *d_table, const sdvl_search_res *d_res,
                          const sdvl_depth_state *d_state, const sdvl_camera *cam, const sdvl_depth_params *fp, TrackPoint *rows, int n_rows,
                          sdvl_depth_out *d_fout, sdvl_depth_out *h_fout, sdvl_depth_out *fout, const DepthMeasureArgs *m = nullptr,
                          uint8_t *out_status = nullptr, const StereoMeasureArgs *sm = nullptr) {
  if (sm)
    SDVL_LAUNCH(ctx, "depth_filter_stereo", depth_filter_stereo_kernel, dim3((n + 127) / 128), dim3(128), d_reqs, d_table, d_res, d_state, n, cam_of(*cam),
                *fp, rows, n_rows, d_fout, h_fout, *sm);
  else if (m)
    SDVL_LAUNCH(ctx, "depth_filter_measured", depth_filter_measured_kernel, dim3((n + 127) / 128), dim3(128), d_reqs, d_table, d_res, d_state, n, cam_of(*cam),
                *fp, rows, n_rows, d_fout, h_fout, *m);
  else
    SDVL_LAUNCH(ctx, "depth_filter", depth_filter_kernel, dim3((n + 127) / 128), dim3(128), d_reqs, d_table, d_res, d_state, n, cam_of(*cam), *fp, rows, n_rows,
                d_fout, h_fout);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  memcpy(fout, h_fout, sizeof(sdvl_depth_out) * static_cast<size_t>(n));
  if (m) memcpy(out_status, m->status_host, static_cast<size_t>(n));
  if (sm) memcpy(out_status, sm->status_host, static_cast<size_t>(n));
  return SDVL_OK;
}

}  // namespace

extern "C" {

// ---- search + depth filter (Map::UpdateCandidates, map.cc:402-498): one submission, one wait
int sdvl_search_run_filter(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                           const sdvl_depth_params *fp, sdvl_track_set *set, sdvl_search_res *out, sdvl_depth_out *fout) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!state || !out || !fout))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (rc) return rc;
  SearchOut so(n);
  const sdvl_part<sdvl_depth_out> d_fout = so.d.take<sdvl_depth_out>(n), h_fout = so.h.take<sdvl_depth_out>(n);
  const SearchReqDev *d_reqs = nullptr;
  const SearchFramePose *d_table = nullptr;
  rc = sdvl_search_enqueue(ctx, n, cam, p, so, &d_reqs, &d_table);
  if (rc) return rc;
  const size_t state_bytes = sizeof(sdvl_depth_state) * static_cast<size_t>(n);  // staged: the states alone
  void *hs = nullptr, *dsx = nullptr;
  rc = sdvl_stage_alloc(ctx, state_bytes, &hs, &dsx);
  if (rc) return rc;
  memcpy(hs, state, state_bytes);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, state_bytes));
  rc = filter_launch_collect(ctx, n, d_reqs, d_table, so.res.cin(ctx->d_out), static_cast<const sdvl_depth_state *>(dsx), cam, fp, rows, n_rows,
                             d_fout.in(ctx->d_out), h_fout.in(ctx->h_out), fout);
  if (rc) return rc;
  memcpy(out, so.h_res.in(ctx->h_out), so.h_res.bytes());
  return SDVL_OK;
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

// ---- the depth filter alone: on search results the caller states.  d_out and h_out: the outcomes
int sdvl_depth_filter(sdvl_ctx *ctx, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                      const double *px, const sdvl_camera *cam, const sdvl_depth_state *state, const sdvl_depth_params *fp,
                      sdvl_track_set *set, sdvl_depth_out *fout) {
  if (!ctx || !cam || !fp || n < 0 || (n > 0 && (!cur_pose || !ref_pose || !bearing || !found || !px || !state || !fout))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (rc) return rc;
  sdvl_layout st, o;
  const StatedStage stated(st, n);
  const sdvl_part<sdvl_depth_out> o_fout = o.take<sdvl_depth_out>(n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_reserve_out_stage(ctx, o.bytes(), st.bytes(), &hs, &ds);
  if (rc) return rc;
  memset(hs, 0, st.bytes());
  stated.fill(hs, n, cur_pose, ref_pose, bearing, found, px, nullptr, state);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  return filter_launch_collect(ctx, n, stated.reqs.cin(ds), stated.tab.cin(ds), stated.res.cin(ds), stated.state.cin(ds), cam, fp, rows, n_rows,
                               o_fout.in(ctx->d_out), o_fout.in(ctx->h_out), fout);
}

// ---- the same two entries for a depth camera
int sdvl_search_run_filter_measured(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                                    const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_depth_job *jobs, int width, int height,
                                    const sdvl_distortion *dist, const sdvl_depth_measure_params *mp, sdvl_search_res *out, sdvl_depth_out *fout,
                                    uint8_t *out_status) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!state || !out || !fout || !out_status))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  DepthMeasure dm;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (!rc) rc = depth_measure_check(ctx, "sdvl_search_run_filter_measured", n, n_jobs, jobs, width, height, cam, dist, mp, &dm);
  if (rc) return rc;
  SearchOut so(n);
  const sdvl_part<sdvl_depth_out> d_fout = so.d.take<sdvl_depth_out>(n), h_fout = so.h.take<sdvl_depth_out>(n);
  const sdvl_part<uint8_t> d_status = so.d.take<uint8_t>(n), h_status = so.h.take<uint8_t>(n);
  const SearchReqDev *d_reqs = nullptr;
  const SearchFramePose *d_table = nullptr;
  rc = sdvl_search_enqueue(ctx, n, cam, p, so, &d_reqs, &d_table);
  if (rc) return rc;
  sdvl_layout st;  // staged: states | jobs | the job of every request
  const sdvl_part<sdvl_depth_state> st_state = st.take<sdvl_depth_state>(n);
  const DepthMeasureStage st_depth(st, n, n_jobs);
  void *hs = nullptr, *dsx = nullptr;
  rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
  if (!rc) rc = st_depth.fill(ctx, hs, n, n_jobs, jobs, width, height);
  if (rc) return rc;
  memcpy(st_state.in(hs), state, st_state.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
  const DepthMeasureArgs m = {st_depth.jobs.cin(dsx), st_depth.req_job.cin(dsx), dm, d_status.in(ctx->d_out), h_status.in(ctx->h_out)};
  rc = filter_launch_collect(ctx, n, d_reqs, d_table, so.res.cin(ctx->d_out), st_state.cin(dsx), cam, fp, rows, n_rows, d_fout.in(ctx->d_out),
                             h_fout.in(ctx->h_out), fout, &m, out_status);
  if (rc) return rc;
  memcpy(out, so.h_res.in(ctx->h_out), so.h_res.bytes());
  return SDVL_OK;
}

// staging as sdvl_depth_filter's, then jobs | the job of every request; d_out and h_out: the outcomes | the status bytes
int sdvl_depth_filter_measured(sdvl_ctx *ctx, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                               const double *px, const int32_t *level, const sdvl_camera *cam, const sdvl_depth_state *state,
                               const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_depth_job *jobs, int width, int height,
                               const sdvl_distortion *dist, const sdvl_depth_measure_params *mp, sdvl_depth_out *fout, uint8_t *out_status) {
  if (!ctx || !cam || !fp || n < 0 || (n > 0 && (!cur_pose || !ref_pose || !bearing || !found || !px || !level || !state || !fout || !out_status)))
    return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  DepthMeasure dm;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (!rc) rc = depth_measure_check(ctx, "sdvl_depth_filter_measured", n, n_jobs, jobs, width, height, cam, dist, mp, &dm);
  if (rc) return rc;
  for (int i = 0; i < n; i++)
    SDVL_REQUIRE(ctx, level[i] >= 0 && level[i] < SDVL_MAX_LEVELS, "sdvl_depth_filter_measured: found level outside 0 .. SDVL_MAX_LEVELS - 1");
  sdvl_layout st, o;
  const StatedStage stated(st, n);
  const DepthMeasureStage st_depth(st, n, n_jobs);
  const sdvl_part<sdvl_depth_out> o_fout = o.take<sdvl_depth_out>(n);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_reserve_out_stage(ctx, o.bytes(), st.bytes(), &hs, &ds);
  if (rc) return rc;
  memset(hs, 0, st.bytes());
  rc = st_depth.fill(ctx, hs, n, n_jobs, jobs, width, height);
  if (rc) return rc;
  stated.fill(hs, n, cur_pose, ref_pose, bearing, found, px, level, state);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  const DepthMeasureArgs m = {st_depth.jobs.cin(ds), st_depth.req_job.cin(ds), dm, o_status.in(ctx->d_out), o_status.in(ctx->h_out)};
  return filter_launch_collect(ctx, n, stated.reqs.cin(ds), stated.tab.cin(ds), stated.res.cin(ds), stated.state.cin(ds), cam, fp, rows, n_rows,
                               o_fout.in(ctx->d_out), o_fout.in(ctx->h_out), fout, &m, out_status);
}

// ---- the same two entries for a stereo rig: the search, stereo_lookup over its results where they lie, the filter's third form — one
// submission, one wait
int sdvl_search_run_filter_stereo(sdvl_ctx *ctx, int n, const sdvl_camera *cam, const sdvl_search_params *p, const sdvl_depth_state *state,
                                  const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_stereo_job *jobs,
                                  const sdvl_stereo_measure_params *mp, sdvl_search_res *out, sdvl_depth_out *fout, uint8_t *out_status) {
  if (!ctx || !cam || !p || !fp || n < 0 || (n > 0 && (!state || !out || !fout || !out_status))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  sdvl_stereo::StereoRule rule;
  size_t lds_bytes = 0;
  double noise_quad = 0.0;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (!rc) rc = stereo_measure_check(ctx, "sdvl_search_run_filter_stereo", n, n_jobs, jobs, cam, mp, &rule, &lds_bytes, &noise_quad);
  if (rc) return rc;
  SearchOut so(n);
  const sdvl_part<sdvl_depth_out> d_fout = so.d.take<sdvl_depth_out>(n), h_fout = so.h.take<sdvl_depth_out>(n);
  const sdvl_part<double> d_z = so.d.take<double>(n);
  const sdvl_part<uint8_t> d_status = so.d.take<uint8_t>(n), h_status = so.h.take<uint8_t>(n);
  const SearchReqDev *d_reqs = nullptr;
  const SearchFramePose *d_table = nullptr;
  rc = sdvl_search_enqueue(ctx, n, cam, p, so, &d_reqs, &d_table);
  if (rc) return rc;
  sdvl_layout st;  // staged: states | jobs | the job of every request
  const sdvl_part<sdvl_depth_state> st_state = st.take<sdvl_depth_state>(n);
  const StereoMeasureStage st_stereo(st, n, n_jobs);
  void *hs = nullptr, *dsx = nullptr;
  rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
  if (!rc) rc = st_stereo.fill(ctx, "sdvl_search_run_filter_stereo", hs, n, n_jobs, jobs);
  if (rc) return rc;
  memcpy(st_state.in(hs), state, st_state.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
  rc = sdvl_stereo_lookup_enqueue(ctx, n, st_stereo.jobs.cin(dsx), so.res.cin(ctx->d_out), st_stereo.req_job.cin(dsx), rule, lds_bytes, d_z.in(ctx->d_out),
                                  d_status.in(ctx->d_out));
  if (rc) return rc;
  const StereoMeasureArgs sm = {d_z.cin(ctx->d_out), d_status.cin(ctx->d_out), noise_quad, h_status.in(ctx->h_out)};
  rc = filter_launch_collect(ctx, n, d_reqs, d_table, so.res.cin(ctx->d_out), st_state.cin(dsx), cam, fp, rows, n_rows, d_fout.in(ctx->d_out),
                             h_fout.in(ctx->h_out), fout, nullptr, out_status, &sm);
  if (rc) return rc;
  memcpy(out, so.h_res.in(ctx->h_out), so.h_res.bytes());
  return SDVL_OK;
}

// staging as sdvl_depth_filter's, then jobs | the job of every request; d_out: the outcomes | z | the status bytes, h_out: the outcomes |
// the status bytes
int sdvl_depth_filter_stereo(sdvl_ctx *ctx, int n, const double *cur_pose, const double *ref_pose, const double *bearing, const int32_t *found,
                             const double *px, const int32_t *level, const sdvl_camera *cam, const sdvl_depth_state *state,
                             const sdvl_depth_params *fp, sdvl_track_set *set, int n_jobs, const sdvl_stereo_job *jobs,
                             const sdvl_stereo_measure_params *mp, sdvl_depth_out *fout, uint8_t *out_status) {
  if (!ctx || !cam || !fp || n < 0 || (n > 0 && (!cur_pose || !ref_pose || !bearing || !found || !px || !level || !state || !fout || !out_status)))
    return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  TrackPoint *rows = nullptr;
  int n_rows = 0;
  sdvl_stereo::StereoRule rule;
  size_t lds_bytes = 0;
  double noise_quad = 0.0;
  int rc = depth_filter_check(ctx, n, state, set, &rows, &n_rows);
  if (!rc) rc = stereo_measure_check(ctx, "sdvl_depth_filter_stereo", n, n_jobs, jobs, cam, mp, &rule, &lds_bytes, &noise_quad);
  if (rc) return rc;
  for (int i = 0; i < n; i++)
    SDVL_REQUIRE(ctx, level[i] >= 0 && level[i] < SDVL_MAX_LEVELS, "sdvl_depth_filter_stereo: found level outside 0 .. SDVL_MAX_LEVELS - 1");
  for (int j = 0; j < n_jobs; j++)
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++)
      SDVL_REQUIRE(ctx, !found[i] || level[i] < jobs[j].left->v.levels, "sdvl_depth_filter_stereo: a hit's level lies outside the left frame's pyramid");
  sdvl_layout st, o;
  const StatedStage stated(st, n);
  const StereoMeasureStage st_stereo(st, n, n_jobs);
  const sdvl_part<sdvl_depth_out> o_fout = o.take<sdvl_depth_out>(n);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n);
  const sdvl_part<double> o_z = o.take<double>(n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_reserve_out_stage(ctx, o.bytes(), st.bytes(), &hs, &ds);
  if (rc) return rc;
  memset(hs, 0, st.bytes());
  rc = st_stereo.fill(ctx, "sdvl_depth_filter_stereo", hs, n, n_jobs, jobs);
  if (rc) return rc;
  stated.fill(hs, n, cur_pose, ref_pose, bearing, found, px, level, state);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  rc = sdvl_stereo_lookup_enqueue(ctx, n, st_stereo.jobs.cin(ds), stated.res.cin(ds), st_stereo.req_job.cin(ds), rule, lds_bytes, o_z.in(ctx->d_out),
                                  o_status.in(ctx->d_out));
  if (rc) return rc;
  const StereoMeasureArgs sm = {o_z.cin(ctx->d_out), o_status.cin(ctx->d_out), noise_quad, o_status.in(ctx->h_out)};
  return filter_launch_collect(ctx, n, stated.reqs.cin(ds), stated.tab.cin(ds), stated.res.cin(ds), stated.state.cin(ds), cam, fp, rows, n_rows,
                               o_fout.in(ctx->d_out), o_fout.in(ctx->h_out), fout, nullptr, out_status, &sm);
}

}  // extern "C"
