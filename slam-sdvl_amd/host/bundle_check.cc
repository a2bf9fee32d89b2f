// bundle_check.cc — the reference's main.cc loop in sequential mode with SDVL::SetBundleAdjustment(true): Map::UpdateMap ends with
// Map::BundleAdjustment (map.cc:130-137) for every keyframe of a map with more than two.  Checks the switch's rules (it throws with a map
// that is no MapperMap and while the mapper thread runs; Start() throws while it is on), that every frame is tracked, that at least one
// window was solved with chi2 not above where it started.  The largest distance of the pose from the rendered trajectory is printed, not
// checked: the adjustment leaves the map's scale free (one fixed keyframe), and nobody has set a bound for that.
//   bundle_check [n_frames]      prints one line; exit code 0 = all checks passed
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "sdvl_host.h"
#undef SDVL_HD
#include "../csrc/sdvl_synth.h"

extern "C" int sdvl_synth_render_host(const sdvl_synth_view *view, int width, int height, uint8_t *out, int stride);

using namespace sdvl;

static const double kCam[4] = {517.3, 516.5, 318.6, 255.3};
static const int W = 640, H = 480;

static SE3 PoseOf(int k) {
  Vector6d xi;
  const double tw[6] = {0.004, 0.002, 0.001, 0.0008, -0.0012, 0.0005};
  for (int q = 0; q < 6; q++) xi.v[q] = tw[q] * k;
  return SE3::Exp(xi);
}

static void Render(int k, std::vector<uint8_t> *px) {
  const SE3 T = PoseOf(k);
  sdvl_synth_view v = {};
  v.fx = kCam[0]; v.fy = kCam[1]; v.u0 = kCam[2]; v.v0 = kCam[3];
  const M3 R = T.GetRotation();
  for (int q = 0; q < 9; q++) v.R[q] = R.m[q];
  const Vector3d t = T.GetTranslation();
  for (int q = 0; q < 3; q++) v.t[q] = t(q);
  v.plane[0] = 0; v.plane[1] = 0; v.plane[2] = 1; v.plane[3] = 2.0;
  v.seed = 20260001;
  v.frame_id = static_cast<uint32_t>(k);
  px->resize(static_cast<size_t>(W) * H);
  sdvl_synth_render_host(&v, W, H, px->data(), W);
}

template <class Fn>
static bool Throws(Fn fn) {
  try {
    fn();
  } catch (const std::runtime_error &) {
    return true;
  }
  return false;
}

int main(int argc, char **argv) {
  const int n_frames = argc > 1 ? std::atoi(argv[1]) : 60;
  Config::GetInstance().SetParameter("SDVL.cell_size", 32);
  Config::GetInstance().SetParameter("SDVL.max_matches", 200);
  Config::GetInstance().SetParameter("SDVL.use_orb", 1);
  Config::GetInstance().SetParameter("SDVL.fast_threshold", 10);
  Config::GetInstance().SetParameter("SDVL.lost_ratio", 0.7);
  Config::GetInstance().SetParameter("SDVL.num_features", 1000);
  int failed = 0;
  try {
    Device dev(0);
    Device::SetCurrent(&dev);
    Camera camera(W, H, kCam[0], kCam[1], kCam[2], kCam[3]);
    {  // the rules of the switch
      PlaneMap stub(Vector3d(0, 0, 1), 2.0);
      SDVL with_stub(&camera, &stub);
      if (!Throws([&] { with_stub.SetBundleAdjustment(true); })) { std::printf("FAIL: no throw without a mapper\n"); failed++; }
      SDVL threaded(&camera);
      threaded.Start();
      if (!Throws([&] { threaded.SetBundleAdjustment(true); })) { std::printf("FAIL: no throw with the mapper thread started\n"); failed++; }
      threaded.Stop();
      threaded.SetBundleAdjustment(true);
      if (!Throws([&] { threaded.Start(); })) { std::printf("FAIL: Start() did not throw with the switch on\n"); failed++; }
      threaded.Stop();
    }
    SDVL handler(&camera);
    handler.SetBundleAdjustment(true);
    MapperMap *map = dynamic_cast<MapperMap *>(handler.GetMap());
    std::vector<uint8_t> px;
    int tracked = 0;
    double pose_err = 0.0;
    for (int k = 0; k < n_frames; k++) {
      Render(k, &px);
      Image img(H, W, CV_8UC1, px.data()), imgu;
      camera.UndistortImage(img, &imgu);  // main.cc:133
      handler.HandleFrame(imgu);          // main.cc:136
      handler.Mapping();                  // main.cc:148-149
      if (k > 0 && handler.GetTrackingQuality() != SDVL::TRACKING_BAD) tracked++;
      double got[7], want[7];
      handler.GetPose().ToArray(got);
      PoseOf(k).Inverse().ToArray(want);  // SDVL::GetPose is camera -> world
      for (int q = 0; q < 7; q++) pose_err = std::max(pose_err, std::fabs(got[q] - want[q]));
    }
    const BundleStats &bs = map->GetBundleStats();
    const bool down = bs.runs > 0 && bs.last.status == SDVL_BUNDLE_OK && bs.last.stage[0].chi2_after <= bs.last.stage[0].chi2_before &&
                      bs.last.stage[1].chi2_after <= bs.last.stage[1].chi2_before;
    std::printf("bundle: frames %d tracked %d keyframes %d runs %ld skipped %ld last window %d free %d fixed %d points %d edges chi2 %.6g -> %.6g | %.6g -> %.6g "
                "pose error %.3g\n", n_frames, tracked, map->GetStats().keyframes, bs.runs, bs.skipped, bs.n_free, bs.n_fixed, bs.n_points, bs.n_edges,
                bs.last.stage[0].chi2_before, bs.last.stage[0].chi2_after, bs.last.stage[1].chi2_before, bs.last.stage[1].chi2_after, pose_err);
    if (tracked != n_frames - 1) { std::printf("FAIL: a frame was not tracked\n"); failed++; }
    if (!down) { std::printf("FAIL: no window solved with chi2 at or below its start\n"); failed++; }
  } catch (const std::exception &e) {
    std::printf("FAIL: %s\n", e.what());
    failed++;
  }
  return failed ? 1 : 0;
}
