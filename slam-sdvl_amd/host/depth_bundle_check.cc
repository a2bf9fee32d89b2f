// depth_bundle_check.cc — the rules of SDVL::SetDepthBundle (depth edges in the local bundle adjustment): it throws without depth seeding,
// without bundle adjustment on, with a map that is no MapperMap, while the mapper thread runs and for a negative or non-finite bf; it is
// accepted in sequential mode behind SetDepthSeeding and SetBundleAdjustment, with and without depth mapping; bf 0 takes 1 / noise_quad of
// the depth mapping; turning the adjustment off turns it off.  tests/test_gpu_depth_bundle_loop.py runs it.
//   depth_bundle_check      prints one line per failure and a summary; exit code 0 = all checks passed
#include <cmath>
#include <cstdio>
#include <limits>
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
    Device dev(0);
    Device::SetCurrent(&dev);
    Camera camera(640, 480, 517.3, 516.5, 318.6, 255.3);
    {
      SDVL plain(&camera);
      MapperMap *m = dynamic_cast<MapperMap *>(plain.GetMap());
      plain.SetBundleAdjustment(true);
      expect(Throws<std::runtime_error>([&] { plain.SetDepthBundle(true); }), "no throw without depth seeding");
      plain.SetBundleAdjustment(false);
      plain.SetDepthSeeding(true);
      expect(Throws<std::runtime_error>([&] { plain.SetDepthBundle(true); }), "no throw without bundle adjustment on");
      plain.SetBundleAdjustment(true);
      expect(!m->DepthBundleOn(), "on before it was told");
      expect(Throws<std::invalid_argument>([&] { plain.SetDepthBundle(true, -1.0); }), "no throw for a negative bf");
      expect(Throws<std::invalid_argument>([&] { plain.SetDepthBundle(true, std::numeric_limits<double>::quiet_NaN()); }), "no throw for a NaN bf");
      expect(Throws<std::invalid_argument>([&] { plain.SetDepthBundle(true, std::numeric_limits<double>::infinity()); }), "no throw for an infinite bf");
      expect(!m->DepthBundleOn(), "a refused call turned it on");
      plain.SetDepthBundle(true);  // depth mapping is not required
      expect(m->DepthBundleOn(), "the switch is not on behind SetDepthSeeding and SetBundleAdjustment");
      expect(std::fabs(m->DepthBundleBf() - 1.0 / 0.0015) < 1e-9, "the default bf is not 1 / 0.0015 without depth mapping");
      plain.SetDepthMapping(true, 0.002, 0.001);
      expect(std::fabs(m->DepthBundleBf() - 1000.0) < 1e-9, "the default bf is not 1 / noise_quad of the depth mapping");
      plain.SetDepthBundle(true, 400.0);
      expect(m->DepthBundleBf() == 400.0, "a given bf is not kept");
      expect(Throws<std::runtime_error>([&] { plain.Start(); }), "Start() did not throw with the adjustment on");
      plain.Stop();
      plain.SetDepthBundle(false);
      expect(!m->DepthBundleOn() && m->BundleAdjustmentOn(), "the switch does not go off alone");
      plain.SetDepthBundle(true);
      plain.SetBundleAdjustment(false);
      expect(!m->DepthBundleOn(), "depth edges stayed on without the adjustment");
    }
    {
      PlaneMap stub(Vector3d(0, 0, 1), 2.0);
      SDVL with_stub(&camera, &stub);
      with_stub.SetDepthSeeding(true);
      expect(Throws<std::runtime_error>([&] { with_stub.SetDepthBundle(true); }), "no throw without a mapper");
    }
    {
      SDVL threaded(&camera);
      threaded.SetDepthSeeding(true);
      threaded.Start();
      expect(Throws<std::runtime_error>([&] { threaded.SetDepthBundle(true); }), "no throw with the mapper thread started");
      threaded.Stop();
    }
  } catch (const std::exception &e) {
    std::printf("FAIL: %s\n", e.what());
    failed++;
  }
  std::printf("depth bundle switch: %d failed\n", failed);
  return failed ? 1 : 0;
}
