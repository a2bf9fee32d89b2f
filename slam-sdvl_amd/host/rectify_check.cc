// rectify_check.cc — the rules of SDVL::SetStereoRectification (stereo rigs as calibrated) from C++, where the mapper thread can be
// started: RectifiedPair::Plan throws std::invalid_argument for a rig the plan refuses; the switch throws without stereo seeding, on a
// camera with a lens of its own, on a camera that is not the pair's, for a baseline that is not the pair's and with the mapper thread
// started; Start() throws while it is on; it goes on and off, SetStereoSeeding(false) and
// SetDepthSeeding(false) take it along, and trackers that share a Camera share it.  Needs a device (tests/test_gpu_rectify.py runs it).
//   rectify_check     prints one line per failure and a summary; exit code 0 = all checks passed
#include <cstdio>
#include <stdexcept>

#include "sdvl_host.h"

using namespace sdvl;

template <class E, class Fn>
static bool Throws(Fn fn) {
  try {
    fn();
  } catch (const E &) {
    return true;
  }
  return false;
}

int main() {
  int failed = 0;
  const auto expect = [&](bool ok, const char *what) {
    if (!ok) {
      std::printf("FAIL: %s\n", what);
      failed++;
    }
  };
  try {
    StereoRig rig;  // config_tum_f1.cfg's camera and lens on both sides, the right camera 0.11 m to the right and turned a little
    const double K[4] = {517.3, 516.5, 318.6, 255.3}, D[5] = {0.2624, -0.9531, -0.0054, 0.0026, 1.1633};
    for (int i = 0; i < 4; i++) rig.K1[i] = rig.K2[i] = K[i];
    for (int i = 0; i < 5; i++) rig.D1[i] = rig.D2[i] = D[i];
    const double R[9] = {0.99984, -0.0050762, -0.016977, 0.0049232, 0.99994699, -0.0090421, 0.017022, 0.0089571, 0.99981499};
    rig.T[0] = -0.11; rig.T[1] = 0.002; rig.T[2] = -0.001;
    expect(Throws<std::invalid_argument>([&] { StereoRig bad = rig; for (int i = 0; i < 9; i++) bad.R[i] = R[i]; RectifiedPair::Plan(bad, 640, 480); }),
           "no throw for an R that is a rotation to five digits only");
    expect(Throws<std::invalid_argument>([&] { StereoRig bad = rig; bad.T[0] = 0.11; RectifiedPair::Plan(bad, 640, 480); }), "no throw for swapped cameras");
    expect(Throws<std::invalid_argument>([&] { RectifiedPair::Plan(rig, 1, 480); }), "no throw for a width of 1");
    const RectifiedPair pair = RectifiedPair::Plan(rig, 640, 480);
    expect(pair.camera().fx == pair.camera().fy && pair.baseline > 0.11 && pair.baseline < 0.1101 && pair.width == 640, "the plan's camera or baseline");
    const sdvl_camera c = pair.camera();
    Camera camera(640, 480, c.fx, c.fy, c.u0, c.v0);
    Device dev(0);
    Device::SetCurrent(&dev);
    {
      SDVL t(&camera);
      expect(Throws<std::runtime_error>([&] { t.SetStereoRectification(pair); }), "no throw without stereo seeding");
      t.SetStereoSeeding(true, 0.11);
      expect(Throws<std::runtime_error>([&] { t.SetStereoRectification(pair); }), "no throw for a baseline that is not the pair's");
      t.SetStereoSeeding(true, pair.baseline);
      t.SetStereoRectification(pair);
      expect(t.StereoRectification() && camera.rectification() != nullptr, "the switch is not on");
      expect(Throws<std::runtime_error>([&] { t.Start(); }), "Start() did not throw with the switch on");
      t.Stop();
      {
        SDVL sharing(&camera);  // a second tracker on the same Camera: the switch is the camera's
        expect(sharing.StereoRectification(), "a tracker that shares the camera does not share the switch");
      }
      t.SetStereoRectification(pair, false);
      expect(!t.StereoRectification() && camera.rectification() == nullptr, "the switch does not go off");
      t.SetStereoRectification(pair);
      t.SetStereoSeeding(false, pair.baseline);
      expect(!t.StereoRectification() && camera.rectification() == nullptr, "SetStereoSeeding(false) left the switch on");
      t.SetStereoSeeding(true, pair.baseline);
      t.SetStereoRectification(pair);
      t.SetDepthSeeding(false);
      expect(!t.StereoSeeding() && !t.StereoRectification() && camera.rectification() == nullptr, "SetDepthSeeding(false) left the switch on");
    }
    {
      Camera lens(640, 480, c.fx, c.fy, c.u0, c.v0);
      SDVL t(&lens);
      t.SetStereoSeeding(true, pair.baseline);
      lens.SetDistortions(D[0], D[1], D[2], D[3], D[4]);
      expect(Throws<std::runtime_error>([&] { t.SetStereoRectification(pair); }), "no throw on a camera with a lens of its own");
    }
    {
      Camera other(640, 480, K[0], K[1], K[2], K[3]);
      SDVL t(&other);
      t.SetStereoSeeding(true, pair.baseline);
      expect(Throws<std::runtime_error>([&] { t.SetStereoRectification(pair); }), "no throw on a camera that is not the pair's");
      Camera small(320, 240, c.fx, c.fy, c.u0, c.v0);
      SDVL s(&small);
      s.SetStereoSeeding(true, pair.baseline);
      expect(Throws<std::runtime_error>([&] { s.SetStereoRectification(pair); }), "no throw on a camera of another size");
    }
    {
      SDVL threaded(&camera);
      threaded.SetStereoSeeding(true, pair.baseline);
      threaded.Start();
      expect(Throws<std::runtime_error>([&] { threaded.SetStereoRectification(pair); }), "no throw with the mapper thread started");
      threaded.Stop();
      threaded.SetStereoRectification(pair);
      threaded.SetStereoRectification(pair, false);
    }
  } catch (const std::exception &e) {
    std::printf("FAIL: %s\n", e.what());
    failed++;
  }
  std::printf("rectify_check: %d failed\n", failed);
  return failed ? 1 : 0;
}
