// depth_map_check.cc — the rules of SDVL::SetDepthMapping (depth cameras inside the reference's mapper): it throws without depth seeding,
// with a map that is no MapperMap, while the mapper thread runs and with the host depth filter selected; Start() throws while it is on;
// and it is accepted in sequential mode behind SetDepthSeeding.  tests/test_gpu_depth_map_loop.py runs it.
//   depth_map_check      prints one line per failure and a summary; exit code 0 = all checks passed
#include <cstdio>
#include <stdexcept>

#include "sdvl_host.h"

using namespace sdvl;

template <class Fn>
static bool Throws(Fn fn) {
  try {
    fn();
  } catch (const std::runtime_error &) {
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
      expect(Throws([&] { plain.SetDepthMapping(true); }), "no throw without depth seeding");
      plain.SetDepthSeeding(true);
      plain.SetDepthMapping(true, 0.002, 0.001);
      expect(dynamic_cast<MapperMap *>(plain.GetMap())->DepthMapping(), "the switch is not on behind SetDepthSeeding");
      expect(Throws([&] { plain.Start(); }), "Start() did not throw with the switch on");
      plain.Stop();
      plain.SetDepthMapping(false);
      expect(!dynamic_cast<MapperMap *>(plain.GetMap())->DepthMapping(), "the switch does not go off");
    }
    {
      PlaneMap stub(Vector3d(0, 0, 1), 2.0);
      SDVL with_stub(&camera, &stub);
      with_stub.SetDepthSeeding(true);
      expect(Throws([&] { with_stub.SetDepthMapping(true); }), "no throw without a mapper");
    }
    {
      SDVL threaded(&camera);
      threaded.SetDepthSeeding(true);
      threaded.Start();
      expect(Throws([&] { threaded.SetDepthMapping(true); }), "no throw with the mapper thread started");
      threaded.Stop();
    }
    {
      SDVL host_filter(&camera);
      host_filter.SetDepthSeeding(true);
      MapperMap::SetDeviceFilter(false);
      expect(Throws([&] { host_filter.SetDepthMapping(true); }), "no throw with the host depth filter");
      MapperMap::SetDeviceFilter(true);
      host_filter.SetDepthMapping(true);
    }
  } catch (const std::exception &e) {
    std::printf("FAIL: %s\n", e.what());
    failed++;
  }
  std::printf("depth mapping switch: %d failed\n", failed);
  return failed ? 1 : 0;
}
