// sdvl_depth_device.h — the depth lookup of include/sdvl_hip.h's "depth cameras" section, stated once for the two kernels that make it:
// depth_seed (sdvl_depth.hip: a keyframe's corners) and depth_filter_measured_kernel (sdvl_depth_filter.hip: the pixel a candidate was found
// at); and what their host entries share: the checks of a job list, the rule's defaults, where an image is read, the job of every item.
#ifndef SDVL_DEPTH_DEVICE_H_
#define SDVL_DEPTH_DEVICE_H_

#include "sdvl_internal.h"

namespace sdvl_depth {

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

// The rule at the level-0 position (fu, fv) of the gray image, window stride s: -> the status, *zc the centre sample in metres.  The
// centre is floor(. + 0.5) of the position, with a lens of the raw pixel its ray lands on (the forward model of cv::undistort, the
// expression undistort_map_kernel evaluates); a whole-numbered position without a lens is its own centre.  The nine loads are issued
// before any of them is looked at; the address of a sample off the image is the centre's, its value ignored.
__device__ __forceinline__ int depth_lookup(const DepthJobDev &job, double fu, double fv, int s, int width, int height, const DepthLens &lens,
                                            const DepthRule &rule, double *zc_out) {
  *zc_out = 0.0;
  if (lens.on) {
    const double x = (fu - lens.u0) / lens.fx, y = (fv - lens.v0) / lens.fy;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = 1 + ((lens.k3 * r2 + lens.k2) * r2 + lens.k1) * r2;
    fu = lens.fx * (x * kr + lens.p1 * _2xy + lens.p2 * (r2 + 2 * x2)) + lens.u0;
    fv = lens.fy * (y * kr + lens.p1 * (r2 + 2 * y2) + lens.p2 * _2xy) + lens.v0;
  }
  fu = floor(fu + 0.5);
  fv = floor(fv + 0.5);
  if (!(fu >= 0.0 && fu < width && fv >= 0.0 && fv < height)) return SDVL_DEPTH_SEED_OUTSIDE;  // (a NaN centre is outside too)
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
  if (!sample_valid(zc, rule)) return SDVL_DEPTH_SEED_HOLE;
  int n_valid = 0;
  double lo = zc, hi = zc;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    if (!(inside[k] && sample_valid(z[k], rule))) continue;
    n_valid++;
    lo = z[k] < lo ? z[k] : lo;
    hi = z[k] > hi ? z[k] : hi;
  }
  if (n_valid < rule.min_valid) return SDVL_DEPTH_SEED_FEW;
  if (hi - lo > rule.edge_ratio * zc) return SDVL_DEPTH_SEED_EDGE;
  *zc_out = zc;
  return SDVL_DEPTH_SEED_OK;
}

}  // namespace sdvl_depth

// ---- host side (sdvl_depth.hip), for every entry that takes a list of sdvl_depth_job.  `who`: the entry's name, in front of a message
// the rule with its defaults (min_depth 0.05: the plane seeding's s > 0.05; no upper limit; 0.05; 6)
int sdvl_depth_rule_of(sdvl_ctx *ctx, const char *who, const sdvl_depth_seed_params *p, sdvl_depth::DepthRule *rule);
// format, stride, scale and range of every job; n: the length of the list the ranges index
int sdvl_depth_jobs_check(sdvl_ctx *ctx, const char *who, int n_jobs, const sdvl_depth_job *jobs, int width, int height, int n);
// where each image is read: HBM and pinned host memory in place; a pageable image as a tight copy in a buffer the context keeps for depth
// images alone (queued on the stream).  Between sdvl_depth_stage_begin and _end an image staged once is not staged again
int sdvl_depth_jobs_resolve(sdvl_ctx *ctx, int n_jobs, const sdvl_depth_job *jobs, int width, int height, sdvl_depth::DepthJobDev *out);
// the copy itself: `height` rows of `row` bytes, `stride` apart at `host`, into one of those buffers (or the one that holds it already);
// sdvl_stereo_depth stages a right image in host memory through it (format SDVL_DEPTH_RIGHT8)
int sdvl_depth_stage_image(sdvl_ctx *ctx, const void *host, long long stride, int format, int width, int height, size_t row, const uint8_t **staged);
sdvl_depth::DepthLens sdvl_depth_lens_of(const sdvl_camera *cam, const sdvl_distortion *dist);
// a call's scope of those buffers: binds the device; outside a sdvl_depth_stage_begin .. _end pair nothing staged earlier stays live
int sdvl_depth_pool_scope(sdvl_ctx *ctx);

// ---- for every entry whose jobs name ranges [c_begin, c_end) of one item list (sdvl_depth_job, sdvl_stereo_job); ranges checked before
// the job of every item of a list of n, -1 for none; where ranges overlap the later job's.  -> whether any did
template <typename Job>
bool sdvl_item_jobs_fill(int n, int n_jobs, const Job *jobs, int32_t *item_job) {
  bool overlap = false;
  for (int i = 0; i < n; i++) item_job[i] = -1;
  for (int j = 0; j < n_jobs; j++)
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++) {
      overlap = overlap || item_job[i] >= 0;
      item_job[i] = j;
    }
  return overlap;
}
// the items of every job whose status is `ok`
template <typename Job>
void sdvl_ok_per_job(int n_jobs, const Job *jobs, const uint8_t *status, int ok, int32_t *ok_per_job) {
  for (int j = 0; j < n_jobs; j++) {
    ok_per_job[j] = 0;
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++) ok_per_job[j] += status[i] == ok ? 1 : 0;
  }
}

#endif  // SDVL_DEPTH_DEVICE_H_
