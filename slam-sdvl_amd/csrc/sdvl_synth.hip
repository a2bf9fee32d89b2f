// sdvl_synth.hip — device build of the synthetic plane-scene generator (sdvl_synth.h): renders n views straight
// into HBM so that bench.py starts its timed region with every input frame already resident; and of the scene with depth
// (sdvl_synth_scene.h) with its per-pixel ground truth.
#include "sdvl_internal.h"
#include "sdvl_synth_scene.h"

namespace {
__global__ __launch_bounds__(256) void synth_render_kernel(const sdvl_synth_view *__restrict__ views, int width, int height,
                                                           uint8_t *__restrict__ out, long long frame_bytes) {
  const sdvl_synth_view view = views[blockIdx.z];
  const int u = blockIdx.x * 64 + (threadIdx.x & 63);
  const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (u >= width || v >= height) return;
  out[static_cast<size_t>(blockIdx.z) * frame_bytes + static_cast<size_t>(v) * width + u] = sdvl_synth_pixel(&view, u, v);
}

// One 64 x 4 tile of one scene per block, one pixel per lane.  The scene record is named by blockIdx.z alone and read in place
// (const __restrict__, 1208 bytes: no per-lane copy): its loads are scalar and the loop over its surfaces has the same trip count in
// every lane; the lanes differ only in the tests on their own hit (sdvl_synth_scene_pixel).  depth / surface: optional, dense per frame.
__global__ __launch_bounds__(256) void synth_render_scene_kernel(const sdvl_synth_scene *__restrict__ scenes, int width, int height,
                                                                 uint8_t *__restrict__ out, long long frame_bytes, float *__restrict__ depth,
                                                                 uint8_t *__restrict__ surface) {
  const sdvl_synth_scene *scene = scenes + blockIdx.z;
  const int u = blockIdx.x * 64 + (threadIdx.x & 63);
  const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (u >= width || v >= height) return;
  float d;
  uint8_t id;
  const uint8_t g = sdvl_synth_scene_pixel(scene, u, v, &d, &id);
  const size_t px = static_cast<size_t>(v) * width + u;
  out[static_cast<size_t>(blockIdx.z) * frame_bytes + px] = g;
  const size_t truth = static_cast<size_t>(blockIdx.z) * width * height + px;
  if (depth) depth[truth] = d;
  if (surface) surface[truth] = id;
}
}  // namespace

extern "C" int sdvl_synth_render(sdvl_ctx *ctx, int n, const sdvl_synth_view *views, int width, int height, void *dev_out,
                                 int64_t frame_bytes) {
  if (!ctx || n < 0 || (n > 0 && (!views || !dev_out))) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, width > 0 && height > 0 && frame_bytes >= static_cast<int64_t>(width) * height, "bad frame geometry");
  SDVL_REQUIRE(ctx, n <= 65535, "at most 65535 views per call");
  const size_t bytes = sizeof(sdvl_synth_view) * n;
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_stage_alloc(ctx, bytes, &hs, &dsx);
  if (rc) return rc;
  memcpy(hs, views, bytes);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, bytes));
  hipLaunchKernelGGL(synth_render_kernel, dim3((width + 63) / 64, (height + 3) / 4, n), dim3(256), 0, ctx->stream,
                     static_cast<const sdvl_synth_view *>(dsx), width, height, static_cast<uint8_t *>(dev_out),
                     static_cast<long long>(frame_bytes));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  return SDVL_OK;
}

extern "C" int sdvl_synth_render_scene(sdvl_ctx *ctx, int n, const sdvl_synth_scene *scenes, int width, int height, void *dev_out,
                                       int64_t frame_bytes, float *dev_depth, uint8_t *dev_surface) {
  if (!ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, n >= 0, "negative number of scenes");
  SDVL_REQUIRE(ctx, n == 0 || (scenes && dev_out), "null scenes or output image");
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, width > 0 && height > 0 && static_cast<int64_t>(height) <= 4 * 65535, "bad frame geometry");
  SDVL_REQUIRE(ctx, frame_bytes >= static_cast<int64_t>(width) * height, "frame_bytes is smaller than one frame");
  SDVL_REQUIRE(ctx, n <= SDVL_SYNTH_SCENE_MAX_VIEWS, "at most SDVL_SYNTH_SCENE_MAX_VIEWS (4096) scenes per call");
  for (int i = 0; i < n; i++) SDVL_REQUIRE(ctx, scenes[i].n_surfaces <= SDVL_SYNTH_MAX_SURFACES, "a scene holds at most SDVL_SYNTH_MAX_SURFACES (8) surfaces");
  const size_t bytes = sizeof(sdvl_synth_scene) * n;
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_stage_alloc(ctx, bytes, &hs, &dsx);
  if (rc) return rc;
  memcpy(hs, scenes, bytes);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, bytes));
  SDVL_LAUNCH(ctx, "synth_render_scene", synth_render_scene_kernel, dim3((width + 63) / 64, (height + 3) / 4, n), dim3(256),
              static_cast<const sdvl_synth_scene *>(dsx), width, height, static_cast<uint8_t *>(dev_out),
              static_cast<long long>(frame_bytes), dev_depth, dev_surface);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  return SDVL_OK;
}

extern "C" int sdvl_synth_scene_size(void) { return static_cast<int>(sizeof(sdvl_synth_scene)); }
extern "C" int sdvl_synth_scene_preset(const char *name, sdvl_synth_scene *out) { return sdvl_synth_scene_fill_preset(name, out); }
extern "C" const char *sdvl_synth_scene_preset_names(void) { return SDVL_SYNTH_SCENE_PRESET_NAMES; }
