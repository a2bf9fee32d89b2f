// sdvl_stereo_device.h — what the entries that take a list of sdvl_stereo_job share (sdvl_stereo.hip states them): sdvl_stereo_depth,
// sdvl_stereo_lookup, and the measured depth filter fed by the matcher (sdvl_depth_filter.hip: sdvl_depth_filter_stereo,
// sdvl_search_run_filter_stereo), whose lookup is the kernel stereo_lookup launched over the results a search left in HBM.
#ifndef SDVL_STEREO_DEVICE_H_
#define SDVL_STEREO_DEVICE_H_

#include "sdvl_depth_device.h"

namespace sdvl_stereo {

struct StereoJobDev {
  const uint8_t *left;   // level 0 of the left frame
  const uint8_t *right;  // device-visible address of the right image
  int32_t lstride, rstride;
  int32_t width, height;
};

struct StereoRule {
  double fb;  // fx x baseline
  int32_t d_lo, d_cap;
  int32_t max_cost;  // 81 x max_sad
  int32_t uniqueness;
  int32_t sw_max;  // the columns of a right strip that the launch's LDS holds
  int32_t pad_;
};

}  // namespace sdvl_stereo

// the rule of `p` with its defaults (0.3 m, no upper limit, 192, 20 per sample, 80) and every refusal of the parameters; sw_max stays 0
int sdvl_stereo_rule_of(sdvl_ctx *ctx, const char *who, const sdvl_camera *cam, const sdvl_stereo_params *p, sdvl_stereo::StereoRule *rule);
// images, context, stride and range of every job; n: the length of the list the ranges index; `item`: what the list holds, for the message
int sdvl_stereo_jobs_check(sdvl_ctx *ctx, const char *who, const char *item, int n_jobs, const sdvl_stereo_job *jobs, int n);
// where each pair is read: a right image in HBM in place, one in host memory as a copy in the buffers the context keeps for depth images
int sdvl_stereo_jobs_resolve(sdvl_ctx *ctx, int n_jobs, const sdvl_stereo_job *jobs, sdvl_stereo::StereoJobDev *out);
// rule->sw_max for windows up to `max_level`, and the dynamic LDS of a launch with it; refuses a strip that does not fit
int sdvl_stereo_lds(sdvl_ctx *ctx, const char *who, int max_level, sdvl_stereo::StereoRule *rule, size_t *lds_bytes);
// stereo_lookup over search results in HBM, queued on the stream: request i with res[i].found and req_job[i] >= 0 is matched at res[i].px
// on res[i].level (clamped to 0 .. SDVL_MAX_LEVELS - 1) against its job; every other request gets status 255 and z 0
int sdvl_stereo_lookup_enqueue(sdvl_ctx *ctx, int n, const sdvl_stereo::StereoJobDev *d_jobs, const sdvl_search_res *d_res, const int32_t *d_req_job,
                               const sdvl_stereo::StereoRule &rule, size_t lds_bytes, double *d_z, uint8_t *d_status);

#endif  // SDVL_STEREO_DEVICE_H_
