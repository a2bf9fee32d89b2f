// A synthetic scene with DEPTH: up to SDVL_SYNTH_MAX_SURFACES textured planar surfaces (unbounded planes or rectangles) seen by the
// camera of sdvl_synth.h.  Every pixel shows the nearest surface its ray hits, textured in the surface's own coordinates (a, b) along
// its axes e1, e2 from its origin, so the sequence has depth steps and occlusion edges for the mapper's triangulation, the depth filter
// and the epipolar search.  Ground truth per pixel: the camera-frame depth of the hit and the index of the surface.
// Same arithmetic contract as sdvl_synth.h (+ - * /, comparisons and sdvl_floor on doubles, -ffp-contract=off): host (synth_host.cc)
// and device (sdvl_synth.hip) give the same bytes.  One unbounded surface with origin 0, e1 = x, e2 = y IS the plane scene of
// sdvl_synth_pixel, byte for byte: (P - 0).e1 = P.x * 1 + P.y * 0 + P.z * 0 adds zeros only.
// The records (sdvl_synth_scene, sdvl_synth_surface) are laid out in include/sdvl_hip.h.
#ifndef SDVL_SYNTH_SCENE_H_
#define SDVL_SYNTH_SCENE_H_

#include "../../include/sdvl_hip.h"
#include "sdvl_synth.h"

// Pixel (u, v) of the scene: its grey level; *depth = the ray parameter k of the nearest hit (the ray has z = 1 in the camera frame, so
// k is the camera-frame z), 0 where nothing is hit; *surface = the index of the surface hit, SDVL_SYNTH_NO_SURFACE where nothing is.
// The loop runs over the record alone (the same trip count and the same loads for every pixel of a view); of its tests only those on
// the pixel's own k and (a, b) differ between pixels.
SDVL_HD inline uint8_t sdvl_synth_scene_pixel(const sdvl_synth_scene *s, int u, int v, float *depth, uint8_t *surface) {
  double rx, ry;
  sdvl_synth_pixel_ray(s->fx, s->fy, s->u0, s->v0, s->dist, u, v, &rx, &ry);
  const double rz = 1.0;
  const double wx = s->R[0] * rx + s->R[3] * ry + s->R[6] * rz;
  const double wy = s->R[1] * rx + s->R[4] * ry + s->R[7] * rz;
  const double wz = s->R[2] * rx + s->R[5] * ry + s->R[8] * rz;
  const double cx = -(s->R[0] * s->t[0] + s->R[3] * s->t[1] + s->R[6] * s->t[2]);
  const double cy = -(s->R[1] * s->t[0] + s->R[4] * s->t[1] + s->R[7] * s->t[2]);
  const double cz = -(s->R[2] * s->t[0] + s->R[5] * s->t[1] + s->R[8] * s->t[2]);
  const uint32_t n = s->n_surfaces < SDVL_SYNTH_MAX_SURFACES ? s->n_surfaces : SDVL_SYNTH_MAX_SURFACES;
  int best = -1;
  double k_best = 0.0, a_best = 0.0, b_best = 0.0;
  uint32_t seed_best = s->seed;
  for (uint32_t i = 0; i < n; i++) {
    const sdvl_synth_surface *f = &s->surfaces[i];
    const double denom = f->plane[0] * wx + f->plane[1] * wy + f->plane[2] * wz;
    const double num = f->plane[3] - (f->plane[0] * cx + f->plane[1] * cy + f->plane[2] * cz);
    if (!(denom > 1e-9 || denom < -1e-9)) continue;  // the ray runs along the surface
    const double k = num / denom;
    if (!(k > 0.0)) continue;                        // behind the camera
    if (best >= 0 && k_best <= k) continue;          // an earlier surface is as near: ties go to the lower index
    const double dx = (cx + k * wx) - f->origin[0], dy = (cy + k * wy) - f->origin[1], dz = (cz + k * wz) - f->origin[2];
    const double a = dx * f->e1[0] + dy * f->e1[1] + dz * f->e1[2];
    const double b = dx * f->e2[0] + dy * f->e2[1] + dz * f->e2[2];
    if (f->half_u > 0.0 && (a > f->half_u || a < -f->half_u)) continue;  // beside the rectangle
    if (f->half_v > 0.0 && (b > f->half_v || b < -f->half_v)) continue;
    best = (int)i; k_best = k; a_best = a; b_best = b; seed_best = s->seed + f->seed_add;
  }
  *depth = best >= 0 ? (float)k_best : 0.0f;
  *surface = best >= 0 ? (uint8_t)best : (uint8_t)SDVL_SYNTH_NO_SURFACE;
  return sdvl_synth_shade(s->texture, seed_best, s->frame_id, best >= 0, a_best, b_best, k_best / s->fx, u, v);
}

// ---- presets (host only): n_surfaces and surfaces of a named scene; camera, pose, seeds, texture and lens stay the caller's
#define SDVL_SYNTH_SCENE_PRESET_NAMES "shelf"

inline void sdvl_synth_scene_set_surface(sdvl_synth_surface *f, uint32_t index, double nx, double ny, double nz, double d, double ox, double oy, double oz,
                                         double e1x, double e1y, double e1z, double half_u, double half_v) {
  f->plane[0] = nx; f->plane[1] = ny; f->plane[2] = nz; f->plane[3] = d;
  f->origin[0] = ox; f->origin[1] = oy; f->origin[2] = oz;
  f->e1[0] = e1x; f->e1[1] = e1y; f->e1[2] = e1z;
  f->e2[0] = 0.0; f->e2[1] = 1.0; f->e2[2] = 0.0;  // every surface so far stands upright
  f->half_u = half_u; f->half_v = half_v;
  f->seed_add = 101u * index;
  f->pad_ = 0;
}

// "shelf": a wall at z = 2 (the plane the trackers bootstrap from) with two boards in front of it at z = 1.5 and z = 1.2 and a third one
// below them, turned by 16.3 degrees about y ((0.28, 0, 0.96) and (0.96, 0, -0.28): an exact Pythagorean pair).  At the identity pose of
// the 640 x 480 TUM camera they cover 71 / 11.6 / 11.6 / 5.8 % of the image.  Returns 0, or -1 for a name that is no preset.
inline int sdvl_synth_scene_fill_preset(const char *name, sdvl_synth_scene *out) {
  if (!name || !out) return -1;
  const char *want = "shelf";
  int q = 0;
  while (name[q] && name[q] == want[q]) q++;
  if (name[q] || want[q]) return -1;
  for (int i = 0; i < SDVL_SYNTH_MAX_SURFACES; i++) out->surfaces[i] = sdvl_synth_surface{};
  out->n_surfaces = 4;
  sdvl_synth_scene_set_surface(&out->surfaces[0], 0, 0.0, 0.0, 1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0);
  sdvl_synth_scene_set_surface(&out->surfaces[1], 1, 0.0, 0.0, 1.0, 1.5, -0.45, -0.2, 1.5, 1.0, 0.0, 0.0, 0.30, 0.25);
  sdvl_synth_scene_set_surface(&out->surfaces[2], 2, 0.0, 0.0, 1.0, 1.2, 0.5, 0.25, 1.2, 1.0, 0.0, 0.0, 0.22, 0.22);
  sdvl_synth_scene_set_surface(&out->surfaces[3], 3, 0.28, 0.0, 0.96, 1.632, 0.0, -0.6, 1.7, 0.96, 0.0, -0.28, 0.35, 0.15);
  return 0;
}

#endif  // SDVL_SYNTH_SCENE_H_
