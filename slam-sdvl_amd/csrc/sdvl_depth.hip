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
// depth_seed: one lane per corner, nine gathers, no LDS; all jobs of a call in one launch.  The nine loads are issued before any of them is
// looked at (addresses of samples off the image are clamped to the centre's, their values ignored).  A keyframe reads ~2.3 k samples of
// a 1.2 MB image: a source in HBM or in pinned host memory is read where it lies; only a pageable source is copied (the context's scratch).
// The file is built with -ffp-contract=off like every other: the centre is the restatement's operation order, ties included.
#include <vector>

#include "sdvl_internal.h"

namespace {

struct DepthJobDev {
  const uint8_t *img;  // device-visible address of the depth image
  long long stride;    // bytes between its rows
  double scale;        // metres per unit (U16)
  int32_t format;
  int32_t pad_;
};

struct DepthLens {
  double fx, fy, u0, v0;
  double k1, k2, p1, p2, k3;
  int32_t on;
  int32_t pad_;
};

struct DepthRule {
  double min_depth, max_depth, edge_ratio;
  int32_t min_valid;
  int32_t pad_;
};

__device__ __forceinline__ double sample_metres(const uint8_t *p, int format, double scale) {
  if (format == SDVL_DEPTH_U16) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);  // (a 16-bit image may start at an odd address)
    return static_cast<double>(v) * scale;
  }
  float v;
  __builtin_memcpy(&v, p, 4);
  return static_cast<double>(v);
}

__device__ __forceinline__ bool sample_valid(double z, const DepthRule &r) {
  // (NaN fails every comparison; +inf fails the first)
  return z <= 1.79769313486231570815e308 && z > 0.0 && z >= r.min_depth && (r.max_depth <= 0.0 || z <= r.max_depth);
}

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
  const DepthJobDev job = jobs[jb];
  const int l = xyl[3 * i + 2], s = 1 << l;
  double fu = static_cast<double>(xyl[3 * i]) * s, fv = static_cast<double>(xyl[3 * i + 1]) * s;
  if (lens.on) {
    const double x = (fu - lens.u0) / lens.fx, y = (fv - lens.v0) / lens.fy;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = 1 + ((lens.k3 * r2 + lens.k2) * r2 + lens.k1) * r2;
    const double u = lens.fx * (x * kr + lens.p1 * _2xy + lens.p2 * (r2 + 2 * x2)) + lens.u0;
    const double v = lens.fy * (y * kr + lens.p1 * (r2 + 2 * y2) + lens.p2 * _2xy) + lens.v0;
    fu = floor(u + 0.5);
    fv = floor(v + 0.5);
  }
  if (!(fu >= 0.0 && fu < width && fv >= 0.0 && fv < height)) {  // (a NaN centre is outside too)
    out_z[i] = 0.0;
    out_status[i] = SDVL_DEPTH_SEED_OUTSIDE;
    return;
  }
  const int cx = static_cast<int>(fu), cy = static_cast<int>(fv);
  const int bps = job.format == SDVL_DEPTH_U16 ? 2 : 4;
  double z[9];
  bool inside[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int sx = cx + (k % 3 - 1) * s, sy = cy + (k / 3 - 1) * s;
    inside[k] = sx >= 0 && sx < width && sy >= 0 && sy < height;
    const int ax = inside[k] ? sx : cx, ay = inside[k] ? sy : cy;  // every address lies inside the image
    z[k] = sample_metres(job.img + ay * job.stride + static_cast<long long>(ax) * bps, job.format, job.scale);
  }
  const double zc = z[4];
  int status = SDVL_DEPTH_SEED_OK;
  if (!sample_valid(zc, rule)) {
    status = SDVL_DEPTH_SEED_HOLE;
  } else {
    int n_valid = 0;
    double lo = zc, hi = zc;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      if (!(inside[k] && sample_valid(z[k], rule))) continue;
      n_valid++;
      lo = z[k] < lo ? z[k] : lo;
      hi = z[k] > hi ? z[k] : hi;
    }
    if (n_valid < rule.min_valid) status = SDVL_DEPTH_SEED_FEW;
    else if (hi - lo > rule.edge_ratio * zc) status = SDVL_DEPTH_SEED_EDGE;
  }
  out_z[i] = status == SDVL_DEPTH_SEED_OK ? zc : 0.0;
  out_status[i] = static_cast<uint8_t>(status);
}

}  // namespace

extern "C" {

int sdvl_depth_seed(sdvl_ctx *ctx, int n_jobs, const sdvl_depth_job *jobs, int width, int height, int n_corners, const int32_t *xyl,
                    const sdvl_camera *cam, const sdvl_distortion *dist, const sdvl_depth_seed_params *p, double *out_z, uint8_t *out_status,
                    int32_t *out_ok_per_job) {
  if (!ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, n_jobs >= 0 && n_corners >= 0, "sdvl_depth_seed: negative count");
  if (n_jobs == 0 || n_corners == 0) {
    for (int j = 0; j < n_jobs && out_ok_per_job; j++) out_ok_per_job[j] = 0;
    return SDVL_OK;
  }
  SDVL_REQUIRE(ctx, jobs && xyl && cam && out_z && out_status && out_ok_per_job, "sdvl_depth_seed: null pointer");
  SDVL_REQUIRE(ctx, width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "sdvl_depth_seed: image size out of range (1 .. 16384 a side)");
  DepthRule rule = {0.05, 0.0, 0.05, 6, 0};  // the plane seeding's s > 0.05; no upper limit
  if (p) {
    SDVL_REQUIRE(ctx, !(p->edge_ratio < 0.0), "sdvl_depth_seed: edge_ratio is negative");
    SDVL_REQUIRE(ctx, p->min_valid >= 0 && p->min_valid <= 9, "sdvl_depth_seed: min_valid outside 1 .. 9");
    if (p->min_depth != 0.0) rule.min_depth = p->min_depth;
    if (p->max_depth != 0.0) rule.max_depth = p->max_depth;
    if (p->edge_ratio != 0.0) rule.edge_ratio = p->edge_ratio;
    if (p->min_valid != 0) rule.min_valid = p->min_valid;
  }
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_depth_job &jb = jobs[j];
    SDVL_REQUIRE(ctx, jb.depth != nullptr, "sdvl_depth_seed: null depth image");
    SDVL_REQUIRE(ctx, jb.format == SDVL_DEPTH_F32 || jb.format == SDVL_DEPTH_U16, "sdvl_depth_seed: unknown depth format");
    const long long bps = jb.format == SDVL_DEPTH_U16 ? 2 : 4;
    SDVL_REQUIRE(ctx, static_cast<long long>(jb.stride) >= width * bps, "sdvl_depth_seed: stride smaller than width x bytes per sample");
    SDVL_REQUIRE(ctx, jb.format != SDVL_DEPTH_U16 || jb.scale > 0.0, "sdvl_depth_seed: a 16-bit depth image needs scale > 0 (metres per unit)");
    SDVL_REQUIRE(ctx, jb.c_begin >= 0 && jb.c_begin <= jb.c_end && jb.c_end <= n_corners, "sdvl_depth_seed: corner range outside the corner list");
  }
  for (int i = 0; i < n_corners; i++)
    SDVL_REQUIRE(ctx, xyl[3 * i + 2] >= 0 && xyl[3 * i + 2] < SDVL_MAX_LEVELS, "sdvl_depth_seed: corner level outside 0 .. SDVL_MAX_LEVELS - 1");
  SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
  // where each image is read: HBM and pinned host memory in place, a pageable image as a tight copy in the context's scratch
  std::vector<const uint8_t *> src(n_jobs);
  std::vector<long long> strides(n_jobs);
  std::vector<int> staged;
  sdvl_layout wk;
  std::vector<sdvl_part<uint8_t>> wk_img(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    strides[j] = jobs[j].stride;
    if (jobs[j].on_device) {
      src[j] = static_cast<const uint8_t *>(jobs[j].depth);
      continue;
    }
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, jobs[j].depth) == hipSuccess && (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeDevice) &&
        attr.devicePointer) {
      src[j] = static_cast<const uint8_t *>(attr.devicePointer);
    } else {
      (void)hipGetLastError();  // an unregistered pointer is not an error here
      const size_t row = static_cast<size_t>(width) * (jobs[j].format == SDVL_DEPTH_U16 ? 2 : 4);
      wk_img[j] = wk.take<uint8_t>(row * height);
      strides[j] = static_cast<long long>(row);
      staged.push_back(j);
    }
  }
  // staging: jobs | corners | the job of every corner (-1: none); d_out and h_out: z | status
  sdvl_layout st, o;
  const sdvl_part<DepthJobDev> st_jobs = st.take<DepthJobDev>(n_jobs);
  const sdvl_part<int32_t> st_xyl = st.take<int32_t>(3 * static_cast<size_t>(n_corners)), st_cj = st.take<int32_t>(n_corners);
  const sdvl_part<double> o_z = o.take<double>(n_corners);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n_corners);
  void *hs = nullptr, *ds = nullptr;
  int rc = sdvl_ensure(ctx, &ctx->d_out, &ctx->d_out_bytes, o.bytes(), false);
  if (!rc) rc = sdvl_ensure(ctx, &ctx->h_out, &ctx->h_out_bytes, o.bytes(), true);
  if (!rc && wk.bytes() > 0) rc = sdvl_ensure(ctx, &ctx->d_work, &ctx->d_work_bytes, wk.bytes(), false);
  if (!rc) rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &ds);
  if (rc) return rc;
  for (int j : staged) {
    uint8_t *d = wk_img[j].in(ctx->d_work);
    SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(d, static_cast<size_t>(strides[j]), jobs[j].depth, jobs[j].stride, static_cast<size_t>(strides[j]), height,
                                         hipMemcpyHostToDevice, ctx->stream));
    src[j] = d;
  }
  DepthJobDev *hj = st_jobs.in(hs);
  int32_t *hcj = st_cj.in(hs);
  for (int i = 0; i < n_corners; i++) hcj[i] = -1;
  for (int j = 0; j < n_jobs; j++) {
    hj[j] = DepthJobDev{src[j], strides[j], jobs[j].scale, jobs[j].format, 0};
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++) hcj[i] = j;
  }
  memcpy(st_xyl.in(hs), xyl, st_xyl.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  DepthLens lens = {cam->fx, cam->fy, cam->u0, cam->v0, 0, 0, 0, 0, 0, 0, 0};
  if (dist && dist->d[0] != 0.0) {  // Camera::SetDistortions tests d0 only (camera.cc:46)
    lens.k1 = dist->d[0]; lens.k2 = dist->d[1]; lens.p1 = dist->d[2]; lens.p2 = dist->d[3]; lens.k3 = dist->d[4];
    lens.on = 1;
  }
  SDVL_LAUNCH(ctx, "depth_seed", depth_seed, dim3((n_corners + 255) / 256), dim3(256), st_jobs.cin(ds), st_xyl.cin(ds), st_cj.cin(ds), n_corners, width,
              height, lens, rule, o_z.in(ctx->d_out), o_status.in(ctx->d_out));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, o.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  memcpy(out_z, o_z.in(ctx->h_out), o_z.bytes());
  memcpy(out_status, o_status.in(ctx->h_out), o_status.bytes());
  for (int j = 0; j < n_jobs; j++) {
    int ok = 0;
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++) ok += out_status[i] == SDVL_DEPTH_SEED_OK ? 1 : 0;
    out_ok_per_job[j] = ok;
  }
  return SDVL_OK;
}

}  // extern "C"
