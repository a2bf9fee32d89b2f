// capi.cc — flat C entry points over the host layer (sdvl_host.h, farm.h) for the Python harness (tests, smoke, bench): B independent
// SDVL trackers on one MI355X stepping together through sdvl::SDVLBatch, and farms of such groups.  A batch handle is an sdvl::TrackerGroup, a farm handle an sdvl::TrackerFarm (farm.h); every entry point casts its handle, makes one
// call and turns an exception into -1 / null plus sdvlh_last_error (the calling thread's own message).
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <set>
#include <string>

#include "farm.h"
#include "homography_init.h"

using namespace sdvl;

namespace {
thread_local std::string g_err;
bool g_use_mapper = false;  // batches and farms created from now on own the reference's mapper instead of the plane map stub

// the body of an entry point that returns a status: 0, or -1 with the exception's message in g_err
template <typename F>
int Guarded(F body) {
  try {
    body();
    return 0;
  } catch (const std::exception &e) {
    g_err = e.what();
    return -1;
  }
}
TrackerGroup *AsGroup(void *bp) { return static_cast<TrackerGroup *>(bp); }
TrackerFarm *AsFarm(void *fp) { return static_cast<TrackerFarm *>(fp); }
}  // namespace

// the records of a step as the Python harness declares them (tracker.py: FrameStats): ten ints, the pose, five ints
typedef FrameStats sdvlh_frame_stats;
static_assert(sizeof(FrameStats) == 120 && offsetof(FrameStats, state) == 0 && offsetof(FrameStats, relocalized) == 36 &&
                  offsetof(FrameStats, pose) == 40 && offsetof(FrameStats, align_features) == 96 && offsetof(FrameStats, host_path) == 112,
              "FrameStats is part of the C API: tracker.py mirrors its layout");

extern "C" {

const char *sdvlh_last_error() { return g_err.c_str(); }

void *sdvlh_device_create(int gpu) {
  try {
    return new Device(gpu);
  } catch (const std::exception &e) {
    g_err = e.what();
    return nullptr;
  }
}
void sdvlh_device_destroy(void *d) { delete static_cast<Device *>(d); }
void *sdvlh_device_ctx(void *d) { return static_cast<Device *>(d)->ctx(); }

int sdvlh_config_set(const char *key, double value) { return Config::GetInstance().SetParameter(key, value) ? 0 : -1; }
int sdvlh_config_read(const char *filename) { return Config::GetInstance().ReadParameters(filename) ? 0 : -1; }
void sdvlh_config_reset() { Config::GetInstance().Reset(); }
// the values a test compares with its own copies of the reference's configuration files: camera block (11) followed by the
// SDVL.* keys those files set: cell_size, min_avg_shift, max_matches, max_keyframes, use_orb, fast_threshold, lost_ratio,
// num_features, min_matches
void sdvlh_config_snapshot(double *out20) {
  const CameraParameters &c = Config::GetCameraParameters();
  const double v[20] = {static_cast<double>(c.width), static_cast<double>(c.height), c.fx, c.fy, c.u0, c.v0, c.d1, c.d2, c.d3, c.d4, c.d5,
                        static_cast<double>(Config::CellSize()), static_cast<double>(Config::MinAvgShift()), static_cast<double>(Config::MaxMatches()),
                        static_cast<double>(Config::MaxKeyframes()), Config::UseORB() ? 1.0 : 0.0, static_cast<double>(Config::FastThreshold()),
                        Config::LostRatio(), static_cast<double>(Config::NumFeatures()), static_cast<double>(Config::MinMatches())};
  for (int i = 0; i < 20; i++) out20[i] = v[i];
}
// test hook: the host build of the sin/cos the ORB kernels use (csrc/sdvl_math.h), same IEEE arithmetic as on the device
void sdvlh_sincos_2pi(double x, double *sn, double *cs) { sincos_2pi(x, sn, cs); }

void *sdvlh_batch_create(void *device, int B, int w, int h, const double *cam4, const double *plane4, const double *first_poses7,
                         int host_threads) {
  try {
    return new TrackerGroup(static_cast<Device *>(device), B, w, h, cam4, plane4, first_poses7, host_threads, g_use_mapper);
  } catch (const std::exception &e) {
    g_err = e.what();
    return nullptr;
  }
}

// TrackerGroup::SetDistortion: the batch's camera gets a lens, the images of every later step are RAW camera frames
int sdvlh_batch_set_distortion(void *bp, const double *dist5) {
  if (!bp || !dist5) return -1;
  return Guarded([&] { AsGroup(bp)->SetDistortion(dist5); });
}

// TrackerGroup::SetColor: the images of every later step are COLOUR camera frames of `format` (enum sdvl_pixel_format, or a raw camera
// format of enum sdvl_raw_format)
int sdvlh_batch_set_color(void *bp, int format) {
  if (!bp) return -1;
  return Guarded([&] { AsGroup(bp)->SetColor(format); });
}

// the trackers of the batch take the reference's two-frame initialisation (SDVL::SetTwoFrameInit) instead of the plane bootstrap; needs
// the reference's mapper (sdvlh_set_mapper(1) before the batch was created)
int sdvlh_batch_set_two_frame_init(void *bp, int on) {
  if (!bp) return -1;
  return Guarded([&] {
    for (int i = 0; i < AsGroup(bp)->size(); i++) AsGroup(bp)->tracker(i).SetTwoFrameInit(on != 0);
  });
}

// the mappers of the batch bundle-adjust every new keyframe (SDVL::SetBundleAdjustment, map.cc:130-137); needs the reference's mapper
// (sdvlh_set_mapper(1) before the batch was created)
int sdvlh_batch_set_bundle_adjustment(void *bp, int on) {
  if (!bp) return -1;
  return Guarded([&] {
    for (int i = 0; i < AsGroup(bp)->size(); i++) AsGroup(bp)->tracker(i).SetBundleAdjustment(on != 0);
  });
}

// tracker i's adjustments so far: counts6 = runs, skipped (windows over SDVL_BUNDLE_MAX_FREE free poses), and the last window's free
// poses, fixed poses, points and edges; *last = its sdvl_bundle_result (zeros before the first run)
int sdvlh_batch_bundle_stats(void *bp, int i, long long *counts6, sdvl_bundle_result *last) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size() || !counts6 || !last) return -1;
  MapperMap *m = dynamic_cast<MapperMap *>(&b->map(i));
  if (!m) return -1;
  const BundleStats &s = m->GetBundleStats();
  counts6[0] = s.runs; counts6[1] = s.skipped; counts6[2] = s.n_free; counts6[3] = s.n_fixed; counts6[4] = s.n_points; counts6[5] = s.n_edges;
  *last = s.last;
  return 0;
}

// the poses (7 doubles each, oldest first) of tracker i's keyframes and their frame ids; returns how many there are (at most cap are written)
int sdvlh_batch_keyframe_poses(void *bp, int i, int cap, double *poses7, int *ids) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size()) return -1;
  const std::vector<std::shared_ptr<Frame>> &kfs = b->map(i).GetKeyframes();
  for (int k = 0; k < static_cast<int>(kfs.size()) && k < cap; k++) {
    kfs[k]->GetPose().ToArray(poses7 + 7 * k);
    ids[k] = kfs[k]->GetID();
  }
  return static_cast<int>(kfs.size());
}

// map mode of the batches and farms created AFTER the call: 0 = plane map stub (every keyframe seeded from the scene plane),
// 1 = the reference's mapper in sequential mode (map.cc; the first keyframe is still bootstrapped from the plane)
void sdvlh_set_mapper(int on) { g_use_mapper = on != 0; }
int sdvlh_batch_map_stats(void *bp, int i, int *out6) {
  MapperMap *m = dynamic_cast<MapperMap *>(&AsGroup(bp)->map(i));
  if (!m) return -1;
  const MapperMap::Stats s = m->GetStats();
  out6[0] = s.candidates; out6[1] = s.converged; out6[2] = s.initialized; out6[3] = s.linked; out6[4] = s.connected; out6[5] = s.keyframes;
  return 0;
}

void sdvlh_batch_destroy(void *bp) { delete AsGroup(bp); }

// Camera::UndistortImage of the host layer (camera.cc:100-105) for one host image; the result comes back to the host
int sdvlh_camera_undistort(void *device, int w, int h, const double *cam4, const double *dist5, const uint8_t *in, int stride, uint8_t *out) {
  try {
    Device *dev = static_cast<Device *>(device);
    Device::SetCurrent(dev);
    Camera cam(w, h, cam4[0], cam4[1], cam4[2], cam4[3]);
    cam.SetDistortions(dist5[0], dist5[1], dist5[2], dist5[3], dist5[4]);
    Image u;
    cam.UndistortImage(Image::Wrap(in, w, h, stride), &u);
    dev->Check(sdvl_device_download(dev->ctx(), u.dev_src, static_cast<int64_t>(w) * h, out), "sdvl_device_download");
    return cam.HasDistortion() ? 1 : 0;
  } catch (const std::exception &e) {
    g_err = e.what();
    return -1;
  }
}

// device-resident tracking tables on (default) / off for the batches stepping from now on; process-wide
void sdvlh_set_track_tables(int on) { SDVLBatch::SetTrackTables(on != 0); }
int sdvlh_track_tables() { return SDVLBatch::TrackTables() ? 1 : 0; }
// the mapper's depth filter on the device (default) or on the host, for the mapper updates from now on; process-wide
void sdvlh_set_device_filter(int on) { MapperMap::SetDeviceFilter(on != 0); }
int sdvlh_device_filter() { return MapperMap::DeviceFilter() ? 1 : 0; }

// test hook: a digest of the map state of tracker i after SyncHostState — the points reachable from its keyframes' features
// (each once): count, sum of Score(), sum of failure counts, deleted ones, sum of inverse depths, sum of GetStd()
int sdvlh_batch_point_digest(void *bp, int i, double *out6) {
  TrackerGroup *b = AsGroup(bp);
  Device::SetCurrent(b->device());
  b->batch().SyncHostState();
  std::set<Point *> seen;
  for (int k = 0; k < 6; k++) out6[k] = 0.0;
  for (auto &kf : b->map(i).GetKeyframes())
    for (auto &ft : kf->GetFeatures()) {
      Point *p = ft ? ft->GetPointRaw() : nullptr;
      if (!p || !seen.insert(p).second) continue;
      out6[0] += 1.0;
      out6[1] += p->Score();
      out6[2] += p->GetFailed();
      out6[3] += p->ToDelete() ? 1.0 : 0.0;
      out6[4] += p->GetInverseDepth();
      out6[5] += p->GetStd();
    }
  return 0;
}

// the live points tracker i's mapper created (MapperMap::GetMapPoints, after SyncHostState): out4 = x y z fixed per point, the rows
// and the order of the oracle's sdvl_ref_tracker_mapper_points.  Returns how many there are (at most cap rows are written; out4 may be
// null with cap 0), or -1 for a tracker on the plane map stub
int sdvlh_batch_map_points(void *bp, int i, int cap, double *out4) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size()) return -1;
  MapperMap *m = dynamic_cast<MapperMap *>(&b->map(i));
  if (!m) return -1;
  int n = -1;
  const int rc = Guarded([&] {
    Device::SetCurrent(b->device());
    b->batch().SyncHostState();
    const std::vector<MapperMap::MapPoint> pts = m->GetMapPoints();
    n = static_cast<int>(pts.size());
    for (int k = 0; k < n && k < cap && out4; k++) {
      out4[4 * k] = pts[k].x; out4[4 * k + 1] = pts[k].y; out4[4 * k + 2] = pts[k].z; out4[4 * k + 3] = pts[k].fixed ? 1.0 : 0.0;
    }
  });
  return rc ? -2 : n;
}

// pose stage on the device (default) or with the host implementation; process-wide
void sdvlh_set_device_pose(int on) { SDVLBatch::SetDevicePose(on != 0); }
int sdvlh_device_pose() { return SDVLBatch::DevicePose() ? 1 : 0; }

// accumulated wall time per SDVLBatch stage (seconds, sdvl::StageId order); returns the number of steps; reset != 0 clears
long sdvlh_batch_stage_times(void *bp, double *out, int cap, int reset) {
  StageTimes &st = AsGroup(bp)->batch().stage_times;
  for (int i = 0; i < cap && i < ST_COUNT; i++) out[i] = st.t[i];
  const long n = st.steps;
  if (reset) st = StageTimes();
  return n;
}

// TrackerGroup::Step on B host pointers (row stride `stride`)
int sdvlh_batch_step_host(void *bp, const uint8_t *const *imgs, int stride, sdvlh_frame_stats *out) {
  return Guarded([&] { AsGroup(bp)->Step(TrackerGroup::Frames::kHost, reinterpret_cast<const void *const *>(imgs), stride, out); });
}
// ... on B device pointers (frames already in HBM) that stay valid while the trackers may still read them
int sdvlh_batch_step_device(void *bp, const void *const *dev_imgs, int stride, sdvlh_frame_stats *out) {
  return Guarded([&] { AsGroup(bp)->Step(TrackerGroup::Frames::kResident, dev_imgs, stride, out); });
}
// ... on B device pointers that are valid for this step only (a slot of an input ring)
int sdvlh_batch_step_device_transient(void *bp, const void *const *dev_imgs, int stride, sdvlh_frame_stats *out) {
  return Guarded([&] { AsGroup(bp)->Step(TrackerGroup::Frames::kTransient, dev_imgs, stride, out); });
}
// TrackerGroup::SetNextImages: the device images the NEXT sdvlh_batch_step_device call will be given (null: none)
int sdvlh_batch_set_next_device(void *bp, const void *const *dev_imgs, int stride) {
  return Guarded([&] { AsGroup(bp)->SetNextImages(dev_imgs, stride); });
}

// ---- depth cameras (SDVL::SetDepthSeeding, TrackerGroup::SetDepth)
// the trackers of the batch seed their keyframes from the depth images handed to the *_depth step calls: format = enum sdvl_depth_format,
// scale = metres per unit of a 16-bit image; the rule's fields as sdvl_depth_seed_params (0: the default)
int sdvlh_batch_set_depth(void *bp, int on, int format, double scale, double edge_ratio, int min_valid, double min_depth, double max_depth) {
  if (!bp) return -1;
  return Guarded([&] { AsGroup(bp)->SetDepth(on != 0, format, scale, sdvl_depth_seed_params{min_depth, max_depth, edge_ratio, min_valid, 0}); });
}
// the step calls with B depth pointers beside the B images (host pointers with _host, device pointers otherwise; dense rows; `depths` or
// single entries may be null)
int sdvlh_batch_step_host_depth(void *bp, const uint8_t *const *imgs, int stride, const void *const *depths, sdvlh_frame_stats *out) {
  return Guarded([&] { AsGroup(bp)->Step(TrackerGroup::Frames::kHost, reinterpret_cast<const void *const *>(imgs), stride, depths, out); });
}
int sdvlh_batch_step_device_depth(void *bp, const void *const *dev_imgs, int stride, const void *const *dev_depths, sdvlh_frame_stats *out) {
  return Guarded([&] { AsGroup(bp)->Step(TrackerGroup::Frames::kResident, dev_imgs, stride, dev_depths, out); });
}
int sdvlh_batch_step_device_transient_depth(void *bp, const void *const *dev_imgs, int stride, const void *const *dev_depths, sdvlh_frame_stats *out) {
  return Guarded([&] { AsGroup(bp)->Step(TrackerGroup::Frames::kTransient, dev_imgs, stride, dev_depths, out); });
}
// the live points tracker i seeded from depth (PlaneMap::GetSeededPoints, after SyncHostState): out7 = x y z keyframe_id u v level per
// point.  Returns how many there are (at most cap rows are written; out7 may be null with cap 0)
int sdvlh_batch_seeded_points(void *bp, int i, int cap, double *out7) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size()) return -1;
  int n = -1;
  const int rc = Guarded([&] {
    Device::SetCurrent(b->device());
    b->batch().SyncHostState();
    const std::vector<PlaneMap::SeededPoint> pts = b->map(i).GetSeededPoints();
    n = static_cast<int>(pts.size());
    for (int k = 0; k < n && k < cap && out7; k++) {
      const double row[7] = {pts[k].x, pts[k].y, pts[k].z, static_cast<double>(pts[k].keyframe_id), static_cast<double>(pts[k].u),
                             static_cast<double>(pts[k].v), static_cast<double>(pts[k].level)};
      std::memcpy(out7 + 7 * k, row, sizeof(row));
    }
  });
  return rc ? -2 : n;
}
// tracker i's depth seeding so far: out8 = keyframes seeded, seeds, corners by status (OK, HOLE, FEW, EDGE, OUTSIDE), keyframes or first
// frames that came without a depth image
int sdvlh_batch_depth_stats(void *bp, int i, long long *out8) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size() || !out8) return -1;
  const PlaneMap::DepthStats &s = b->map(i).GetDepthStats();
  out8[0] = s.keyframes; out8[1] = s.seeds;
  for (int k = 0; k < 5; k++) out8[2 + k] = s.by_status[k];
  out8[7] = s.no_depth;
  return 0;
}
// ---- stereo cameras (SDVL::SetStereoSeeding, TrackerGroup::SetStereo): the pointers the *_depth step calls take beside the images are
// the pairs' rectified right images (8-bit gray, dense rows); the rule's fields as sdvl_stereo_params (0: the default)
int sdvlh_batch_set_stereo(void *bp, int on, double baseline, double min_depth, double max_depth, int max_disparity, int max_sad, int uniqueness) {
  if (!bp) return -1;
  return Guarded([&] { AsGroup(bp)->SetStereo(on != 0, baseline, sdvl_stereo_params{0.0, min_depth, max_depth, max_disparity, max_sad, uniqueness, 0, nullptr}); });
}
// tracker i's stereo seeding so far: out8 = keyframes seeded, seeds, corners by status (OK, NOMATCH, AMBIGUOUS, EDGE, OUTSIDE), keyframes
// or first frames that came without a right image — the counters of sdvlh_batch_depth_stats under the stereo producer's names
int sdvlh_batch_stereo_stats(void *bp, int i, long long *out8) { return sdvlh_batch_depth_stats(bp, i, out8); }
// Depth cameras inside the mappers of the batch (SDVL::SetDepthMapping): needs sdvlh_batch_set_depth and the reference's mapper; the
// trackers share the noise parameters (0: the defaults)
int sdvlh_batch_set_depth_mapping(void *bp, int on, double noise_abs, double noise_quad) {
  if (!bp) return -1;
  return Guarded([&] {
    for (int i = 0; i < AsGroup(bp)->size(); i++) AsGroup(bp)->tracker(i).SetDepthMapping(on != 0, noise_abs, noise_quad);
  });
}
// tracker i's depth mapping so far: out9 = candidate updates measured, fallen back by status (HOLE, FEW, EDGE, OUTSIDE), keyframes looked
// up, corners fixed and matched, fixed and unmatched, linked
int sdvlh_batch_depth_map_stats(void *bp, int i, long long *out9) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size() || !out9) return -1;
  MapperMap *m = dynamic_cast<MapperMap *>(&b->map(i));
  if (!m) return -1;
  const MapperMap::DepthMapStats &s = m->GetDepthMapStats();
  out9[0] = s.measured;
  for (int k = 0; k < 4; k++) out9[1 + k] = s.fallback[k];
  out9[5] = s.keyframes; out9[6] = s.fixed_matched; out9[7] = s.fixed_unmatched; out9[8] = s.linked;
  return 0;
}
// ---- stereo cameras inside the mappers of the batch (SDVL::SetStereoMapping): needs sdvlh_batch_set_stereo and the reference's mapper;
// the trackers share disparity_sigma (pixels; 0: 0.25, not measured against a real pair)
int sdvlh_batch_set_stereo_mapping(void *bp, int on, double disparity_sigma) {
  if (!bp) return -1;
  return Guarded([&] { AsGroup(bp)->SetStereoMapping(on != 0, disparity_sigma); });
}
// ---- stereo rigs as calibrated (SDVL::SetStereoRectification): rig30 = K1[4] D1[5] K2[4] D2[5] R[9] T[3] with X_right = R X_left + T.
// The rig is planned for the batch's image size (sdvl_stereo_rectify_plan) and the step calls then take the RAW images of both cameras.
// out5 (if not null) = the rectified camera fx fy u0 v0 and the baseline: the batch must have been made with that camera, and
// sdvlh_batch_set_stereo called with that baseline.  on = 0 turns the switch off.  plan_only = 1: out5 is filled and nothing is set
int sdvlh_batch_set_stereo_rectification(void *bp, int on, const double *rig30, int plan_only, double *out5) {
  if (!bp || (on && !rig30)) return -1;
  return Guarded([&] {
    TrackerGroup *g = AsGroup(bp);
    if (!on) {
      g->SetStereoRectification(RectifiedPair(), false);
      return;
    }
    StereoRig rig;
    const double *p = rig30;
    for (int i = 0; i < 4; i++) rig.K1[i] = *p++;
    for (int i = 0; i < 5; i++) rig.D1[i] = *p++;
    for (int i = 0; i < 4; i++) rig.K2[i] = *p++;
    for (int i = 0; i < 5; i++) rig.D2[i] = *p++;
    for (int i = 0; i < 9; i++) rig.R[i] = *p++;
    for (int i = 0; i < 3; i++) rig.T[i] = *p++;
    const RectifiedPair pair = RectifiedPair::Plan(rig, g->width(), g->height());
    if (out5) {
      out5[0] = pair.camera().fx; out5[1] = pair.camera().fy; out5[2] = pair.camera().u0; out5[3] = pair.camera().v0;
      out5[4] = pair.baseline;
    }
    if (!plan_only) g->SetStereoRectification(pair, true);
  });
}
// tracker i's stereo mapping so far: out9 = candidate updates measured, fallen back by status (NOMATCH, AMBIGUOUS, EDGE, OUTSIDE),
// keyframes matched, corners fixed and matched, fixed and unmatched, linked — the counters of sdvlh_batch_depth_map_stats under the
// stereo producer's names
int sdvlh_batch_stereo_map_stats(void *bp, int i, long long *out9) { return sdvlh_batch_depth_map_stats(bp, i, out9); }

// Depth edges in the mappers' bundle adjustment (SDVL::SetDepthBundle): needs sdvlh_batch_set_depth and sdvlh_batch_set_bundle_adjustment;
// bf in pixel x metres, 0: the default; the trackers share it
int sdvlh_batch_set_depth_bundle(void *bp, int on, double bf) {
  if (!bp) return -1;
  return Guarded([&] {
    for (int i = 0; i < AsGroup(bp)->size(); i++) AsGroup(bp)->tracker(i).SetDepthBundle(on != 0, bf);
  });
}
// tracker i's depth edges so far: out13 = lookups by status (OK, HOLE, FEW, EDGE, OUTSIDE), observations that got a depth stored, then
// edges, edges with a depth and depth edges that ended on level 1 of the last window, the same three summed over all windows, and the
// features that were handed to the lookup
int sdvlh_batch_depth_bundle_stats(void *bp, int i, long long *out13) {
  TrackerGroup *b = AsGroup(bp);
  if (!b || i < 0 || i >= b->size() || !out13) return -1;
  MapperMap *m = dynamic_cast<MapperMap *>(&b->map(i));
  if (!m) return -1;
  const DepthBundleStats &s = m->GetDepthBundleStats();
  for (int k = 0; k < 5; k++) out13[k] = s.lookups[k];
  out13[5] = s.stored;
  out13[6] = s.last_edges; out13[7] = s.last_depth_edges; out13[8] = s.last_depth_level1;
  out13[9] = s.total_edges; out13[10] = s.total_depth_edges; out13[11] = s.total_depth_level1;
  out13[12] = s.features;
  return 0;
}

// ---- TrackerFarm (farm.h): G groups x Bg sequences on ONE GPU
void *sdvlh_farm_create(int gpu, int G, int Bg, int w, int h, const double *cam4, const double *plane4, const double *first_poses7,
                        int host_threads_per_group) {
  try {
    return new TrackerFarm(gpu, G, Bg, w, h, cam4, plane4, first_poses7, host_threads_per_group, g_use_mapper);
  } catch (const std::exception &e) {
    g_err = e.what();
    return nullptr;
  }
}
void sdvlh_farm_destroy(void *fp) { delete AsFarm(fp); }
void sdvlh_farm_set_fibers(void *fp, int n) { AsFarm(fp)->SetFibers(n); }
void sdvlh_farm_set_host_input(void *fp, int on) { AsFarm(fp)->SetHostInput(on != 0); }
void sdvlh_farm_set_input_ring(void *fp, int on) { AsFarm(fp)->SetInputRing(on != 0); }
int sdvlh_farm_set_color(void *fp, int format) {
  if (!fp) return -1;
  return Guarded([&] { AsFarm(fp)->SetColor(format); });
}
int sdvlh_farm_reserve(void *fp, int frames_per_group) {
  return Guarded([&] { AsFarm(fp)->Reserve(frames_per_group); });
}
void *sdvlh_farm_ctx(void *fp, int g) { return AsFarm(fp)->device(g).ctx(); }
void *sdvlh_farm_batch(void *fp, int g) { return &AsFarm(fp)->group(g); }  // a handle for the sdvlh_batch_* calls; the farm keeps it

// TrackerFarm::FeedStats of the last host-fed run: seconds inside sdvl_feed_images, seconds waiting for a free ring slot, transfers,
// seconds the workers waited for their step's transfer to be issued and to arrive (summed over groups), group-steps that began
// before their images had arrived, seconds the feeder waited for its own earlier transfers
void sdvlh_farm_feed_stats(void *fp, double *out6) {
  const TrackerFarm::FeedStats s = AsFarm(fp)->feed_stats();
  out6[0] = s.feed_call_s;
  out6[1] = s.feed_wait_s;
  out6[2] = static_cast<double>(s.feed_calls);
  out6[3] = s.work_wait_s + s.arrive_wait_s;
  out6[4] = static_cast<double>(s.late_acquires);
  out6[5] = s.feed_throttle_s;
}

// TrackerFarm::Run: n_steps steps with `workers` host threads (0 = one per group).  Returns 0, or -1 with the run's first failure in
// sdvlh_last_error.
int sdvlh_farm_run(void *fp, int n_steps, const void *const *dev_frames, int stride, sdvlh_frame_stats *out, int workers) {
  return Guarded([&] { AsFarm(fp)->Run(n_steps, dev_frames, stride, out, workers); });
}

// ---- two-frame initialisation, the host arithmetic behind the device stages (homography_init.h)
// src / dst [n][2] of HomographyInit::ComputeHomography (homography_init.cc:243-250) for tracked pixels: the input of sdvl_homography_ransac
int sdvlh_homography_matches(int n, const float *pixels1, const float *pixels2, const double *cam4, double *src, double *dst) {
  if (n < 0 || !cam4 || (n > 0 && (!pixels1 || !pixels2 || !src || !dst))) return -1;
  HomographyMath h(cam4, 0.0, 1.0);
  h.SetTracks(n, pixels1, pixels2);
  std::memcpy(src, h.Src().data(), sizeof(double) * 2 * n);
  std::memcpy(dst, h.Dst().data(), sizeof(double) * 2 * n);
  return 0;
}
// ComputeHomography from the RANSAC's inliers on, and the scaling of InitSecondFrame.  out_R9 / out_t3: frame 1 -> frame 2, scaled;
// out_counts4 = {inliers of CheckInliers, inliers of CheckDecompositionInliers, visibility score 0, visibility score 1};
// out_inliers [n] and out_tri [n][3] may be null.  1 = initialised, 0 = refused (homography_init.cc:99-103), -1 = bad argument
int sdvlh_homography_from_inliers(int n, const float *pixels1, const float *pixels2, const double *cam4, double inlier_error_threshold,
                                  double map_scale, int min_init_corners, int n_ransac_inliers, const int32_t *ransac_inliers, double *out_H9,
                                  double *out_R9, double *out_t3, int32_t *out_counts4, double *out_depth, int32_t *out_inliers, double *out_tri) {
  if (n <= 0 || !pixels1 || !pixels2 || !cam4 || !ransac_inliers || !out_H9 || !out_R9 || !out_t3 || !out_counts4 || !out_depth) return -1;
  HomographyMath h(cam4, inlier_error_threshold, map_scale);
  h.SetTracks(n, pixels1, pixels2);
  const bool ok = h.ComputeHomography(n_ransac_inliers, ransac_inliers, min_init_corners);
  std::memcpy(out_H9, h.BestH(), sizeof(double) * 9);
  std::memcpy(out_R9, h.Rotation(), sizeof(double) * 9);
  std::memcpy(out_t3, h.Translation(), sizeof(double) * 3);
  out_counts4[0] = h.NumHomographyInliers();
  out_counts4[1] = static_cast<int32_t>(h.Inliers().size());
  out_counts4[2] = h.VisibilityScore(0);
  out_counts4[3] = h.VisibilityScore(1);
  *out_depth = h.MedianDepth();
  if (out_inliers) std::copy(h.Inliers().begin(), h.Inliers().end(), out_inliers);
  if (out_tri && !h.Triangulations().empty()) std::memcpy(out_tri, h.Triangulations().data(), sizeof(double) * 3 * n);
  return ok ? 1 : 0;
}
// test hooks: the two Jacobi routines
void sdvlh_jacobi_eigen_sym(int n, double *A, double *V, double *eig) { JacobiEigenSym(n, A, V, eig); }
void sdvlh_jacobi_svd3(const double *A, double *U, double *s, double *V) { JacobiSvd3(A, U, s, V); }

}  // extern "C"
