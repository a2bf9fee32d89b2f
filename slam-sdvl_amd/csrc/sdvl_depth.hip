// sdvl_depth.hip — depth camera input: the depth of a keyframe's filtered corners, read from a registered depth image (sdvl_depth_seed).
// Map::InitCandidates carries a `fixed` branch that makes a candidate a fixed point at a known depth (map.cc:269,385-389); the reference
// never feeds it.  The rule is this project's own and tests/depth_seed_restatement.py is its specification:
//   centre    the level-0 pixel (X, Y) = (x << l, y << l) of a corner; with a lens the gray image was undistorted but the depth image lies on
//             the RAW grid, so the centre sample is the raw pixel the corner's ray lands on — the forward model of cv::undistort, the
//             expression undistort_map_kernel evaluates (sdvl_undistort.hip), rounded half up
//   window    the nine samples at (cx + i s, cy + j s), i, j in {-1, 0, 1}, s = 1 << l: the localisation of a level-l corner
//   valid     inside the image, finite, > 0, >= min_depth, <= max_depth (when there is one)
//   status    the first that applies of OUTSIDE (centre off the image), HOLE (centre invalid), FEW (fewer than min_valid valid samples),
//             EDGE (max - min over the valid samples > edge_ratio x the centre's depth); otherwise OK and z = the centre sample, unfiltered
// depth_seed: one lane per corner, nine gathers, no LDS; all jobs of a call in one launch.  The lookup itself (depth_lookup,
// sdvl_depth_device.h) is shared with the mapper's measured depth filter (sdvl_depth_filter.hip) and with sdvl_depth_lookup below, which applies it
// at the sub-pixel position a feature was found at (the depths bundle adjustment's depth edges carry).  A keyframe reads ~2.3 k samples of a 1.2 MB
// image: a source in HBM or in pinned host memory is read where it lies; only a pageable source is copied, into buffers the context keeps
// for depth images alone.  The file is built with -ffp-contract=off like every other: the centre is the restatement's operation order,
// ties included.
#include <string>
#include <vector>

#include "sdvl_depth_device.h"

using namespace sdvl_depth;

namespace {

__global__ __launch_bounds__(256) void depth_seed(const DepthJobDev *__restrict__ jobs, const int32_t *__restrict__ xyl, const int32_t *__restrict__ corner_job,
                                                  int n, int width, int height, DepthLens lens, DepthRule rule, double *__restrict__ out_z,
                                                  uint8_t *__restrict__ out_status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int jb = corner_job[i];
  if (jb < 0) {  // a corner no job names
    out_z[i] = 0.0;
    out_status[i] = SDVL_DEPTH_SEED_HOLE;
    return;
  }
  const int l = xyl[3 * i + 2], s = 1 << l;
  double zc;
  const int status = depth_lookup(jobs[jb], static_cast<double>(xyl[3 * i]) * s, static_cast<double>(xyl[3 * i + 1]) * s, s, width, height, lens, rule, &zc);
  out_z[i] = zc;
  out_status[i] = static_cast<uint8_t>(status);
}

// sdvl_depth_lookup: the same rule at a position of its own, one lane per position — the level-0 pixel a feature was found at and the
// stride of the level it was found on, as depth_filter_measured_kernel (sdvl_depth_filter.hip) applies it
__global__ __launch_bounds__(256) void depth_lookup_kernel(const DepthJobDev *__restrict__ jobs, const double *__restrict__ px2, const int32_t *__restrict__ level,
                                                           const int32_t *__restrict__ pos_job, int n, int width, int height, DepthLens lens, DepthRule rule,
                                                           double *__restrict__ out_z, uint8_t *__restrict__ out_status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int jb = pos_job[i];
  if (jb < 0) {  // a position no job names
    out_z[i] = 0.0;
    out_status[i] = SDVL_DEPTH_SEED_HOLE;
    return;
  }
  double zc;
  const int status = depth_lookup(jobs[jb], px2[2 * i], px2[2 * i + 1], 1 << level[i], width, height, lens, rule, &zc);
  out_z[i] = zc;
  out_status[i] = static_cast<uint8_t>(status);
}

// ---- sdvl_depth_seed and sdvl_depth_lookup: one body (depth_items_run) over what each states of its own — its inputs, their parts of the
// staging block and how they are filled, the level of an item with the message of its check, and its launch (tail: the arguments the two
// kernels share behind n)
struct SeedStage {  // staging: jobs | corners | the job of every corner (-1: none)
  static constexpr const char *who = "sdvl_depth_seed", *level_msg = "sdvl_depth_seed: corner level outside 0 .. SDVL_MAX_LEVELS - 1";
  const int32_t *xyl;
  sdvl_part<int32_t> st_xyl;
  bool stated() const { return xyl != nullptr; }
  int level(int i) const { return xyl[3 * i + 2]; }
  void take(sdvl_layout &st, int n) { st_xyl = st.take<int32_t>(3 * static_cast<size_t>(n)); }
  void fill(void *hs) const { memcpy(st_xyl.in(hs), xyl, st_xyl.bytes()); }
  template <typename... Tail>
  void launch(sdvl_ctx *ctx, const void *ds, const DepthJobDev *jobs, const int32_t *item_job, int n, Tail... tail) const {
    SDVL_LAUNCH(ctx, "depth_seed", depth_seed, dim3((n + 255) / 256), dim3(256), jobs, st_xyl.cin(ds), item_job, n, tail...);
  }
};

struct LookupStage {  // staging: jobs | positions | levels | the job of every position (-1: none)
  static constexpr const char *who = "sdvl_depth_lookup", *level_msg = "sdvl_depth_lookup: level outside 0 .. SDVL_MAX_LEVELS - 1";
  const double *px2;
  const int32_t *lv;
  sdvl_part<double> st_px;
  sdvl_part<int32_t> st_level;
  bool stated() const { return px2 != nullptr && lv != nullptr; }
  int level(int i) const { return lv[i]; }
  void take(sdvl_layout &st, int n) { st_px = st.take<double>(2 * static_cast<size_t>(n)), st_level = st.take<int32_t>(n); }
  void fill(void *hs) const { memcpy(st_px.in(hs), px2, st_px.bytes()), memcpy(st_level.in(hs), lv, st_level.bytes()); }
  template <typename... Tail>
  void launch(sdvl_ctx *ctx, const void *ds, const DepthJobDev *jobs, const int32_t *item_job, int n, Tail... tail) const {
    SDVL_LAUNCH(ctx, "depth_lookup", depth_lookup_kernel, dim3((n + 255) / 256), dim3(256), jobs, st_px.cin(ds), st_level.cin(ds), item_job, n, tail...);
  }
};

// d_out and h_out: z | status
template <typename Stage>
int depth_items_run(sdvl_ctx *ctx, Stage &stage, int n_jobs, const sdvl_depth_job *jobs, int width, int height, int n, const sdvl_camera *cam,
                    const sdvl_distortion *dist, const sdvl_depth_seed_params *p, double *out_z, uint8_t *out_status, int32_t *out_ok_per_job) {
  if (!ctx) return SDVL_ERR_INVALID;
  const std::string w(Stage::who);
  SDVL_REQUIRE(ctx, n_jobs >= 0 && n >= 0, w + ": negative count");
  if (n_jobs == 0 || n == 0) {
    for (int j = 0; j < n_jobs && out_ok_per_job; j++) out_ok_per_job[j] = 0;
    return SDVL_OK;
  }
  SDVL_REQUIRE(ctx, jobs && stage.stated() && cam && out_z && out_status && out_ok_per_job, w + ": null pointer");
  DepthRule rule;
  int rc = sdvl_depth_rule_of(ctx, Stage::who, p, &rule);
  if (!rc) rc = sdvl_depth_jobs_check(ctx, Stage::who, n_jobs, jobs, width, height, n);
  if (rc) return rc;
  for (int i = 0; i < n; i++) SDVL_REQUIRE(ctx, stage.level(i) >= 0 && stage.level(i) < SDVL_MAX_LEVELS, Stage::level_msg);
  sdvl_layout st, o;
  const sdvl_part<DepthJobDev> st_jobs = st.take<DepthJobDev>(n_jobs);
  stage.take(st, n);
  const sdvl_part<int32_t> st_item_job = st.take<int32_t>(n);
  const sdvl_part<double> o_z = o.take<double>(n);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_reserve_out_stage(ctx, o.bytes(), st.bytes(), &hs, &ds);
  if (!rc) rc = sdvl_depth_jobs_resolve(ctx, n_jobs, jobs, width, height, st_jobs.in(hs));
  if (rc) return rc;
  sdvl_item_jobs_fill(n, n_jobs, jobs, st_item_job.in(hs));  // (ranges that overlap: the later job's)
  stage.fill(hs);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  stage.launch(ctx, ds, st_jobs.cin(ds), st_item_job.cin(ds), n, width, height, sdvl_depth_lens_of(cam, dist), rule, o_z.in(ctx->d_out), o_status.in(ctx->d_out));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  rc = sdvl_collect_out(ctx, o.bytes());
  if (rc) return rc;
  memcpy(out_z, o_z.in(ctx->h_out), o_z.bytes());
  memcpy(out_status, o_status.in(ctx->h_out), o_status.bytes());
  sdvl_ok_per_job(n_jobs, jobs, out_status, SDVL_DEPTH_SEED_OK, out_ok_per_job);
  return SDVL_OK;
}

}  // namespace

// ---- what the entries that take depth jobs share (sdvl_depth_device.h)
int sdvl_depth_rule_of(sdvl_ctx *ctx, const char *who, const sdvl_depth_seed_params *p, DepthRule *rule) {
  *rule = DepthRule{0.05, 0.0, 0.05, 6, 0};
  if (!p) return SDVL_OK;
  const std::string w(who);
  SDVL_REQUIRE(ctx, !(p->edge_ratio < 0.0), w + ": edge_ratio is negative");
  SDVL_REQUIRE(ctx, p->min_valid >= 0 && p->min_valid <= 9, w + ": min_valid outside 1 .. 9");
  if (p->min_depth != 0.0) rule->min_depth = p->min_depth;
  if (p->max_depth != 0.0) rule->max_depth = p->max_depth;
  if (p->edge_ratio != 0.0) rule->edge_ratio = p->edge_ratio;
  if (p->min_valid != 0) rule->min_valid = p->min_valid;
  return SDVL_OK;
}

int sdvl_depth_jobs_check(sdvl_ctx *ctx, const char *who, int n_jobs, const sdvl_depth_job *jobs, int width, int height, int n) {
  const std::string w(who);
  SDVL_REQUIRE(ctx, width >= 1 && height >= 1 && width <= 16384 && height <= 16384, w + ": image size out of range (1 .. 16384 a side)");
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_depth_job &jb = jobs[j];
    SDVL_REQUIRE(ctx, jb.depth != nullptr, w + ": null depth image");
    SDVL_REQUIRE(ctx, jb.format != SDVL_DEPTH_RIGHT8, w + ": unknown depth format: a right image (SDVL_DEPTH_RIGHT8) is no depth image, sdvl_stereo_depth reads it");
    SDVL_REQUIRE(ctx, jb.format == SDVL_DEPTH_F32 || jb.format == SDVL_DEPTH_U16, w + ": unknown depth format");
    const long long bps = jb.format == SDVL_DEPTH_U16 ? 2 : 4;
    SDVL_REQUIRE(ctx, static_cast<long long>(jb.stride) >= width * bps, w + ": stride smaller than width x bytes per sample");
    SDVL_REQUIRE(ctx, jb.format != SDVL_DEPTH_U16 || jb.scale > 0.0, w + ": a 16-bit depth image needs scale > 0 (metres per unit)");
    SDVL_REQUIRE(ctx, jb.c_begin >= 0 && jb.c_begin <= jb.c_end && jb.c_end <= n, w + ": corner range outside the corner list");
  }
  return SDVL_OK;
}

DepthLens sdvl_depth_lens_of(const sdvl_camera *cam, const sdvl_distortion *dist) {
  DepthLens lens = {cam->fx, cam->fy, cam->u0, cam->v0, 0, 0, 0, 0, 0, 0, 0};
  if (dist && dist->d[0] != 0.0) {  // Camera::SetDistortions tests d0 only (camera.cc:46)
    lens.k1 = dist->d[0]; lens.k2 = dist->d[1]; lens.p1 = dist->d[2]; lens.p2 = dist->d[3]; lens.k3 = dist->d[4];
    lens.on = 1;
  }
  return lens;
}

// The copies of pageable depth images live in buffers of their own, so that no scratch of a search (d_work) is written while a submission
// reads it.  A buffer keeps its allocation from call to call; `live` says that it holds `host` as staged since sdvl_depth_stage_begin
// (outside a begin .. end pair: since the start of this call).
int sdvl_depth_jobs_resolve(sdvl_ctx *ctx, int n_jobs, const sdvl_depth_job *jobs, int width, int height, DepthJobDev *out) {
  const int scope = sdvl_depth_pool_scope(ctx);
  if (scope) return scope;
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_depth_job &jb = jobs[j];
    out[j] = DepthJobDev{static_cast<const uint8_t *>(jb.depth), jb.stride, jb.scale, jb.format, 0};
    if (jb.on_device) continue;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, jb.depth) == hipSuccess && (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeDevice) &&
        attr.devicePointer) {
      out[j].img = static_cast<const uint8_t *>(attr.devicePointer);
      continue;
    }
    (void)hipGetLastError();  // an unregistered pointer is not an error here
    const size_t row = static_cast<size_t>(width) * (jb.format == SDVL_DEPTH_U16 ? 2 : 4);
    const int rc = sdvl_depth_stage_image(ctx, jb.depth, jb.stride, jb.format, width, height, row, &out[j].img);
    if (rc) return rc;
    out[j].stride = static_cast<long long>(row);
  }
  return SDVL_OK;
}

int sdvl_depth_pool_scope(sdvl_ctx *ctx) {
  SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
  if (!ctx->depth_stage_open)
    for (sdvl_ctx::DepthStaged &e : ctx->depth_pool) e.live = 0;
  return SDVL_OK;
}

int sdvl_depth_stage_image(sdvl_ctx *ctx, const void *host, long long stride, int format, int width, int height, size_t row, const uint8_t **staged) {
  const size_t bytes = row * height;
  int hit = -1, spare = -1;
  for (size_t k = 0; k < ctx->depth_pool.size(); k++) {
    const sdvl_ctx::DepthStaged &e = ctx->depth_pool[k];
    if (e.live && e.host == host && e.stride == stride && e.format == format && e.width == width && e.height == height) hit = static_cast<int>(k);
    if (!e.live && e.bytes >= bytes && (spare < 0 || e.bytes < ctx->depth_pool[spare].bytes)) spare = static_cast<int>(k);
  }
  if (hit < 0) {
    if (spare < 0) {
      void *d = nullptr;
      SDVL_HIP_CHECK(ctx, hipMalloc(&d, bytes));
      ctx->depth_pool.push_back(sdvl_ctx::DepthStaged{d, bytes, nullptr, 0, 0, 0, 0, 0});
      spare = static_cast<int>(ctx->depth_pool.size()) - 1;
    }
    sdvl_ctx::DepthStaged &e = ctx->depth_pool[spare];
    SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(e.d, row, host, stride, row, height, hipMemcpyHostToDevice, ctx->stream));
    e.host = host; e.stride = stride; e.format = format; e.width = width; e.height = height;
    e.live = 1;
    hit = spare;
  }
  *staged = static_cast<const uint8_t *>(ctx->depth_pool[hit].d);
  return SDVL_OK;
}

extern "C" {

int sdvl_depth_stage_begin(sdvl_ctx *ctx) {
  if (!ctx) return SDVL_ERR_INVALID;
  for (sdvl_ctx::DepthStaged &e : ctx->depth_pool) e.live = 0;
  ctx->depth_stage_open = 1;
  return SDVL_OK;
}

int sdvl_depth_stage_end(sdvl_ctx *ctx) {
  if (!ctx) return SDVL_ERR_INVALID;
  for (sdvl_ctx::DepthStaged &e : ctx->depth_pool) e.live = 0;
  ctx->depth_stage_open = 0;
  return SDVL_OK;
}

int sdvl_depth_seed(sdvl_ctx *ctx, int n_jobs, const sdvl_depth_job *jobs, int width, int height, int n_corners, const int32_t *xyl,
                    const sdvl_camera *cam, const sdvl_distortion *dist, const sdvl_depth_seed_params *p, double *out_z, uint8_t *out_status,
                    int32_t *out_ok_per_job) {
  SeedStage stage{xyl, {}};
  return depth_items_run(ctx, stage, n_jobs, jobs, width, height, n_corners, cam, dist, p, out_z, out_status, out_ok_per_job);
}

int sdvl_depth_lookup(sdvl_ctx *ctx, int n_jobs, const sdvl_depth_job *jobs, int width, int height, int n, const double *px2, const int32_t *level,
                      const sdvl_camera *cam, const sdvl_distortion *dist, const sdvl_depth_seed_params *p, double *out_z, uint8_t *out_status,
                      int32_t *out_ok_per_job) {
  LookupStage stage{px2, level, {}, {}};
  return depth_items_run(ctx, stage, n_jobs, jobs, width, height, n, cam, dist, p, out_z, out_status, out_ok_per_job);
}

}  // extern "C"
