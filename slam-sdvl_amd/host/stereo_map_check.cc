// stereo_map_check.cc — the rules of SDVL::SetStereoMapping (stereo cameras inside the reference's mapper).  The mapper's half needs no
// device: MapperMap::SetStereoMapping throws with the host depth filter selected, together with depth mapping, for a disparity_sigma that
// is negative or not finite and for an fx x baseline that is not positive; Start() throws while it is on; SetDepthMapping throws while it
// is on; and the switch goes on and off.  The tracker's half (--device; tests/test_gpu_stereo_map_loop.py runs it): it throws without
// stereo seeding, with a map that is no MapperMap and while the mapper thread runs; SetStereoSeeding(false) and SetDepthSeeding(false)
// throw while it is on.  tests/test_stereo_lookup_restatement_cpu.py runs the mapper's half.
//   stereo_map_check [--device]     prints one line per failure and a summary; exit code 0 = all checks passed
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main(int argc, char **argv) {
  const bool with_device = argc > 1 && std::strcmp(argv[1], "--device") == 0;
  int failed = 0;
  const auto expect = [&](bool ok, const char *what) {
    if (!ok) {
      std::printf("FAIL: %s\n", what);
      failed++;
    }
  };
  const double fb = 517.3 * 0.11, nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  try {
    Camera camera(640, 480, 517.3, 516.5, 318.6, 255.3);
    {
      MapperMap m(Vector3d(0, 0, 1), 2.0, &camera);
      expect(!m.StereoMapping() && !m.Measuring(), "the switch is on by default");
      expect(Throws<std::invalid_argument>([&] { m.SetStereoMapping(true, -0.1, fb); }), "no throw for a negative disparity_sigma");
      expect(Throws<std::invalid_argument>([&] { m.SetStereoMapping(true, nan, fb); }), "no throw for a NaN disparity_sigma");
      expect(Throws<std::invalid_argument>([&] { m.SetStereoMapping(true, inf, fb); }), "no throw for an infinite disparity_sigma");
      expect(Throws<std::invalid_argument>([&] { m.SetStereoMapping(true, 0.25, 0.0); }), "no throw for fx x baseline 0");
      expect(!m.StereoMapping(), "a refused call turned the switch on");
      m.SetStereoMapping(true, 0.0, fb);
      expect(m.StereoMapping() && m.Measuring() && !m.DepthMapping() && m.DisparitySigma() == 0.0, "the switch is not on");
      expect(Throws<std::runtime_error>([&] { m.Start(); }), "Start() did not throw with the switch on");
      expect(!m.IsThreaded(), "Start() started the thread with the switch on");
      expect(Throws<std::runtime_error>([&] { m.SetDepthMapping(true); }), "SetDepthMapping did not throw with stereo mapping on");
      m.SetStereoMapping(true, 0.5, fb);
      expect(m.DisparitySigma() == 0.5, "the second call's disparity_sigma is not kept");
      m.SetStereoMapping(false, 0.0, fb);
      expect(!m.StereoMapping() && !m.Measuring(), "the switch does not go off");
      MapperMap::SetDeviceFilter(false);
      expect(Throws<std::runtime_error>([&] { m.SetStereoMapping(true, 0.25, fb); }), "no throw with the host depth filter");
      MapperMap::SetDeviceFilter(true);
      m.SetDepthMapping(true, 0.002, 0.001);
      expect(Throws<std::runtime_error>([&] { m.SetStereoMapping(true, 0.25, fb); }), "no throw with depth mapping on");
      m.SetDepthMapping(false);
      m.SetStereoMapping(true, 0.25, fb);
      m.SetStereoMapping(false, 0.0, fb);
    }
    if (with_device) {
      Device dev(0);
      Device::SetCurrent(&dev);
      {
        SDVL plain(&camera);
        expect(Throws<std::runtime_error>([&] { plain.SetStereoMapping(true); }), "no throw without stereo seeding");
        plain.SetDepthSeeding(true);
        expect(Throws<std::runtime_error>([&] { plain.SetStereoMapping(true); }), "no throw behind depth seeding from a depth image");
        plain.SetDepthSeeding(false);
        plain.SetStereoSeeding(true, 0.11);
        expect(Throws<std::invalid_argument>([&] { plain.SetStereoMapping(true, -1.0); }), "no throw for a negative disparity_sigma");
        plain.SetStereoMapping(true, 0.3);
        expect(dynamic_cast<MapperMap *>(plain.GetMap())->StereoMapping(), "the switch is not on behind SetStereoSeeding");
        expect(Throws<std::runtime_error>([&] { plain.Start(); }), "Start() did not throw with the switch on");
        plain.Stop();
        expect(Throws<std::runtime_error>([&] { plain.SetStereoSeeding(false, 0.11); }), "SetStereoSeeding(false) did not throw with the switch on");
        expect(Throws<std::runtime_error>([&] { plain.SetDepthSeeding(false); }), "SetDepthSeeding(false) did not throw with the switch on");
        expect(Throws<std::runtime_error>([&] { plain.SetDepthMapping(true); }), "SetDepthMapping did not throw behind stereo seeding");
        expect(plain.StereoSeeding(), "a refused call turned stereo seeding off");
        plain.SetStereoMapping(false);
        expect(!dynamic_cast<MapperMap *>(plain.GetMap())->StereoMapping(), "the switch does not go off");
        plain.SetStereoSeeding(false, 0.11);
      }
      {
        PlaneMap stub(Vector3d(0, 0, 1), 2.0);
        SDVL with_stub(&camera, &stub);
        with_stub.SetStereoSeeding(true, 0.11);
        expect(Throws<std::runtime_error>([&] { with_stub.SetStereoMapping(true); }), "no throw without a mapper");
      }
      {
        SDVL threaded(&camera);
        threaded.SetStereoSeeding(true, 0.11);
        threaded.Start();
        expect(Throws<std::runtime_error>([&] { threaded.SetStereoMapping(true); }), "no throw with the mapper thread started");
        threaded.Stop();
      }
      {
        SDVL host_filter(&camera);
        host_filter.SetStereoSeeding(true, 0.11);
        MapperMap::SetDeviceFilter(false);
        expect(Throws<std::runtime_error>([&] { host_filter.SetStereoMapping(true); }), "no throw with the host depth filter");
        MapperMap::SetDeviceFilter(true);
        host_filter.SetStereoMapping(true);
      }
    }
  } catch (const std::exception &e) {
    std::printf("FAIL: %s\n", e.what());
    failed++;
  }
  std::printf("stereo mapping switch (%s): %d failed\n", with_device ? "mapper and tracker" : "mapper", failed);
  return failed ? 1 : 0;
}
