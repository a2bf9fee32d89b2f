// Host build of the synthetic sequence generator (sdvl_synth.h, sdvl_synth_scene.h) -> libsdvl_synth.so, used by the CPU tests.
#include "sdvl_synth_scene.h"

extern "C" int sdvl_synth_render_host(const sdvl_synth_view *view, int width, int height, uint8_t *out, int stride) {
  for (int v = 0; v < height; v++)
    for (int u = 0; u < width; u++) out[(long)v * stride + u] = sdvl_synth_pixel(view, u, v);
  return 0;
}

// The host twin of sdvl_synth_render_scene for one scene: image rows `stride` bytes apart; depth (float) and surface (uint8) are optional
// and dense (row stride = width).  -1: a null scene or image, a frame without pixels, a stride below the width or more surfaces than a
// scene holds.
extern "C" int sdvl_synth_render_scene_host(const sdvl_synth_scene *scene, int width, int height, uint8_t *out, int stride, float *depth,
                                            uint8_t *surface) {
  if (!scene || !out || width <= 0 || height <= 0 || stride < width || scene->n_surfaces > SDVL_SYNTH_MAX_SURFACES) return -1;
  for (int v = 0; v < height; v++)
    for (int u = 0; u < width; u++) {
      float d;
      uint8_t id;
      out[(long)v * stride + u] = sdvl_synth_scene_pixel(scene, u, v, &d, &id);
      if (depth) depth[(long)v * width + u] = d;
      if (surface) surface[(long)v * width + u] = id;
    }
  return 0;
}

extern "C" int sdvl_synth_scene_size(void) { return (int)sizeof(sdvl_synth_scene); }
extern "C" int sdvl_synth_scene_preset(const char *name, sdvl_synth_scene *out) { return sdvl_synth_scene_fill_preset(name, out); }
extern "C" const char *sdvl_synth_scene_preset_names(void) { return SDVL_SYNTH_SCENE_PRESET_NAMES; }
