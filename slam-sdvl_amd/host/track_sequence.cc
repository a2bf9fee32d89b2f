// track_sequence.cc — the per-frame loop of the reference's main.cc:89-171 on the MI355X front-end, in plain C++ against
// sdvl_host.h: read (or render) a frame, undistort it, SDVL::HandleFrame(), print the pose.  It is the "maintainer's
// view" of the drop-in: nothing here knows about HIP; the classes are the reference's (Camera, Config, SDVL, Map).
//
//   track_sequence --synthetic N [--seed S]                      N frames of the S-A scene, rendered on the host
//   track_sequence --list frames.txt                             one binary PGM (P5, 8 bit) or PPM (P6, 8 bit RGB: converted to gray on the
//                                                                device, SDVL_RGB8) path per line, e.g. a TUM / EuRoC list
//   track_sequence --list frames.txt --raw-format NAME           the P5 files are RAW camera frames of that format (raw Bayer is commonly stored as PGM), converted
//                                                                to gray on the device: bayer_rggb | bayer_grbg | bayer_gbrg | bayer_bggr (a mosaic, named by its
//                                                                top-left 2x2 tile), yuyv | uyvy, gray10 | gray12 | gray16 (little-endian).  With a two-byte format
//                                                                a P5 of width 2 W carries a W-pixel frame.  16-bit PGM (maxval > 255) is big-endian: unsupported
//   track_sequence --synthetic N --scene shelf                   N frames of a scene with depth (csrc/sdvl_synth_scene.h: several surfaces, nearest hit) instead of
//                                                                the one plane; the map still bootstraps from --plane (the default is the scene's wall)
//   track_sequence --synthetic N --scene shelf --depth           a depth camera: every frame comes with the renderer's registered depth image and the
//                                                                keyframes' points are seeded from it (SDVL::SetDepthSeeding) — no plane; a --plane is ignored
//   ... --depth --depth-mapping                                  the depth camera inside the reference's mapper too (SDVL::SetDepthMapping; implies --mapper): every tracked
//                                                                frame's depth feeds the candidates' filter, new keyframes' corners become fixed points; beside --depth only
//   track_sequence --list frames.txt --depth-list depth.txt --depth-scale S   the same from disk: one 16-bit binary PGM (P5, maxval above 255; netpbm's samples are
//                                                                big-endian and are swapped here) per frame, S metres per unit (TUM: 0.0002)
//   track_sequence --synthetic N --scene shelf --stereo --baseline B   a stereo camera: every frame comes with the rendered right image — the right camera's centre is the
//                                                                left one's plus B metres along the left camera's x axis, the same orientation — and the keyframes' points
//                                                                are seeded from the pair (SDVL::SetStereoSeeding) — no plane; a --plane is ignored
//   ... --stereo --stereo-mapping [--disparity-sigma X]          the stereo pair inside the reference's mapper too (SDVL::SetStereoMapping; implies --mapper): every tracked
//                                                                frame's right image feeds the candidates' filter through the matcher at the found pixel, new keyframes'
//                                                                corners become fixed points; X: the disparity noise in pixels (default 0.25, not measured against a real pair)
//   track_sequence --list frames.txt --right-list right.txt --baseline B   the same from disk: one 8-bit binary PGM, the rectified right image, per frame
//   ... --stereo --rig FILE                                      a stereo rig as calibrated (SDVL::SetStereoRectification): FILE is a settings file in the configuration
//                                                                file's form with the RIGHT camera's Camera.fx fy u0 v0 d1..d5 and Rig.r11 .. Rig.r33, Rig.tx ty tz
//                                                                (X_right = R X_left + T; R defaults to the identity); the left camera and its lens are the main
//                                                                configuration's (--cam, --dist).  The rig is planned, the tracker's camera is the plan's rectified
//                                                                camera, and the frames of both cameras are RAW: with --synthetic N --scene NAME both views are rendered
//                                                                through their lenses, the right one at R, T; with --list / --right-list they are the files'.  The
//                                                                baseline is the plan's |T| (--baseline is not needed); poses are the rectified left camera's
//   track_sequence ... --depth --depth-bundle [--depth-bf X]  depth edges in the local bundle adjustment (SDVL::SetDepthBundle; implies --bundle): X in
//                                                                pixel x metres, default 1 / noise_quad of the depth mapping = 666.7
//   common:  [--config file.cfg] [--size W H] [--cam fx fy u0 v0] [--dist d0 d1 d2 d3 d4] [--plane nx ny nz d] [--mapper] [--bundle] [--init plane|two-frame]
//   round 5 (bench.py's latency legs):  [--texture plane|camera]  [--trackers N]  N cameras = N host threads, each with its own Device
//            (= HIP stream), Camera, Map and SDVL, all fed the same frames;  [--batch]  with --trackers N: the N cameras step together through
//            ONE sdvl::SDVLBatch::HandleFrames call per frame on one thread and one stream (the batched form of the same call);  [--prerender]  the synthetic frames are rendered on the GPU
//            into page-locked host memory before the loop (the window of main.cc:136-138 never contained the rendering anyway; this keeps
//            a 300-frame run short);  [--pageable]  with --prerender: plain malloc'ed frames, what an unregistered cv::Mat is;
//            [--lookahead]  the loop undistorts frame k + 1 before it tracks frame k and names it with SDVL::SetNextImage (a sequence from
//            disk is there before it is needed): its pyramid and corners are built while the host finishes frame k;
//            [--set SDVL.key value]  a configuration value (after --config);  [--quiet]  no per-frame lines;  [--json]  one JSON line with the rates;  [--profile]  per-kernel dispatch time and host stages
//
// --init plane (the default): the first frame becomes a keyframe whose points are seeded on the plane n.X = d (world = first camera),
// which is exact for the synthetic scene and a stand-in for real data.  --init two-frame: the reference's two-frame homography
// initialisation (SDVL::SetTwoFrameInit; implies --mapper): the tracker starts from the camera alone.
// Output: one line per frame  "k state quality matches attempts inliers  qw qx qy qz tx ty tz"  and the tracked frames/s of
// the HandleFrame calls alone (the window of main.cc:136-138).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "sdvl_host.h"
#undef SDVL_HD  // sdvl_math.h and sdvl_synth.h each define their own host/device qualifier macro
#include "../csrc/sdvl_synth_scene.h"

extern "C" int sdvl_synth_render_host(const sdvl_synth_view *view, int width, int height, uint8_t *out, int stride);
extern "C" int sdvl_synth_render_scene_host(const sdvl_synth_scene *scene, int width, int height, uint8_t *out, int stride, float *depth, uint8_t *surface);

using namespace sdvl;

namespace {

// binary PGM (P5: gray) or PPM (P6: RGB byte order), 8 bit; *format = PIX_GRAY8 / PIX_RGB8
bool ReadPNM(const std::string &path, int *w, int *h, std::vector<uint8_t> *px, int *format) {
  std::ifstream f(path, std::ios::binary);
  std::string magic;
  if (!(f >> magic) || (magic != "P5" && magic != "P6")) return false;
  const int channels = magic == "P6" ? 3 : 1;
  *format = magic == "P6" ? PIX_RGB8 : PIX_GRAY8;
  int vals[3], n = 0;
  while (n < 3) {  // width, height, maxval with '#' comments in between
    f >> std::ws;
    if (f.peek() == '#') { std::string skip; std::getline(f, skip); continue; }
    if (!(f >> vals[n])) return false;
    n++;
  }
  if (vals[2] != 255) return false;
  f.get();  // the single whitespace byte after maxval
  *w = vals[0];
  *h = vals[1];
  px->resize(static_cast<size_t>(vals[0]) * vals[1] * channels);
  f.read(reinterpret_cast<char *>(px->data()), static_cast<std::streamsize>(px->size()));
  return static_cast<size_t>(f.gcount()) == px->size();
}

// a depth image: binary PGM (P5) with 16-bit samples (maxval above 255), which netpbm stores big-endian: swapped to the machine's order
bool ReadDepthPGM(const std::string &path, int *w, int *h, std::vector<uint16_t> *px) {
  std::ifstream f(path, std::ios::binary);
  std::string magic;
  if (!(f >> magic) || magic != "P5") return false;
  int vals[3], n = 0;
  while (n < 3) {
    f >> std::ws;
    if (f.peek() == '#') { std::string skip; std::getline(f, skip); continue; }
    if (!(f >> vals[n])) return false;
    n++;
  }
  if (vals[2] <= 255 || vals[2] > 65535 || vals[0] <= 0 || vals[1] <= 0) return false;
  f.get();
  *w = vals[0];
  *h = vals[1];
  std::vector<uint8_t> bytes(static_cast<size_t>(vals[0]) * vals[1] * 2);
  f.read(reinterpret_cast<char *>(bytes.data()), static_cast<std::streamsize>(bytes.size()));
  if (static_cast<size_t>(f.gcount()) != bytes.size()) return false;
  px->resize(bytes.size() / 2);
  for (size_t i = 0; i < px->size(); i++) (*px)[i] = static_cast<uint16_t>((bytes[2 * i] << 8) | bytes[2 * i + 1]);
  return true;
}

// --rig FILE: the right camera and the rig's R, T in the configuration file's form (Config::ReadKeyValues)
bool ReadRig(const std::string &path, StereoRig *rig, std::string *err) {
  static const char *const cam_keys[9] = {"Camera.fx", "Camera.fy", "Camera.u0", "Camera.v0", "Camera.d1", "Camera.d2", "Camera.d3", "Camera.d4", "Camera.d5"};
  static const char *const r_keys[9] = {"Rig.r11", "Rig.r12", "Rig.r13", "Rig.r21", "Rig.r22", "Rig.r23", "Rig.r31", "Rig.r32", "Rig.r33"};
  static const char *const t_keys[3] = {"Rig.tx", "Rig.ty", "Rig.tz"};
  bool have_cam[4] = {false, false, false, false}, have_t[3] = {false, false, false};
  const bool opened = Config::ReadKeyValues(path, [&](const std::string &key, double v) {
    bool known = false;
    for (int i = 0; i < 9; i++) {
      if (key == cam_keys[i]) { (i < 4 ? rig->K2[i] : rig->D2[i - 4]) = v; if (i < 4) have_cam[i] = true; known = true; }
      if (key == r_keys[i]) { rig->R[i] = v; known = true; }
    }
    for (int i = 0; i < 3; i++)
      if (key == t_keys[i]) { rig->T[i] = v; have_t[i] = true; known = true; }
    if (!known && err->empty()) *err = path + ": unknown key " + key;
  });
  if (!opened) { *err = "cannot read " + path; return false; }
  if (!err->empty()) return false;
  for (int i = 0; i < 4; i++)
    if (!have_cam[i]) { *err = path + ": the right camera needs Camera.fx, Camera.fy, Camera.u0 and Camera.v0"; return false; }
  for (int i = 0; i < 3; i++)
    if (!have_t[i]) { *err = path + ": the rig needs Rig.tx, Rig.ty and Rig.tz"; return false; }
  return true;
}

// --raw-format NAME -> PIX_* (0: no such name)
int RawFormatByName(const std::string &name) {
  static const char *const names[] = {"bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr", "yuyv", "uyvy", "gray10", "gray12", "gray16"};
  for (int i = 0; i < 9; i++)
    if (name == names[i]) return PIX_BAYER_RGGB8 + i;
  return 0;
}

const char kUsage[] =
    "track_sequence --synthetic N [--seed S] [--scene NAME [--depth | --stereo --baseline B]] |\n"
    "               --list frames.txt [--raw-format NAME] [--depth-list depth.txt --depth-scale S | --right-list right.txt --baseline B]\n"
    "  --list: one binary PGM (P5, 8 bit) or PPM (P6, 8 bit RGB) path per line\n"
    "  --raw-format NAME: the P5 files are raw camera frames, converted to gray on the device:\n"
    "      bayer_rggb | bayer_grbg | bayer_gbrg | bayer_bggr   a Bayer mosaic, named by the 2x2 tile at its top-left corner\n"
    "      yuyv | uyvy                                         YUV 4:2:2; the P5 is 2 W bytes wide for a W-pixel frame\n"
    "      gray10 | gray12 | gray16                            little-endian 16-bit gray; the P5 is 2 W bytes wide\n"
    "    16-bit PGM (maxval above 255) is big-endian and is not supported\n"
    "  --depth: with --synthetic N --scene NAME, the keyframes' points are seeded from the renderer's registered depth image (no plane)\n"
    "  --depth-bundle [--depth-bf X]: with --depth, observations that carry a measured depth are depth edges of the bundle adjustment (implies --bundle)\n"
    "  --depth-list FILE --depth-scale S: one 16-bit P5 depth image (big-endian samples, S metres per unit) per frame of --list\n"
    "  --stereo --baseline B: with --synthetic N --scene NAME, a stereo camera: every frame comes with the rendered right image (the right camera's\n"
    "      centre is the left one's plus B metres along the left camera's x axis, the same orientation) and the keyframes' points are seeded from the\n"
    "      pair (no plane, no lens)\n"
    "  --stereo-mapping [--disparity-sigma X]: with --stereo, the right image of every tracked frame feeds the mapper's depth filter and new\n"
    "      keyframes' corners become fixed points (implies --mapper); X: disparity noise in pixels, default 0.25 (not measured against a real pair)\n"
    "  --right-list FILE --baseline B: one 8-bit P5 rectified right image per frame of --list\n"
    "  --rig FILE: with --stereo, a rig as calibrated: FILE holds the right camera's Camera.fx fy u0 v0 d1..d5 and Rig.r11 .. r33, Rig.tx ty tz\n"
    "      (X_right = R X_left + T) in the configuration file's form; the left camera is --cam / --dist.  Both cameras' frames are raw and are\n"
    "      rectified on the device; the baseline is the rig's\n"
    "  common: [--config file.cfg] [--size W H] [--cam fx fy u0 v0] [--dist d0 d1 d2 d3 d4] [--plane nx ny nz d] [--mapper] [--bundle]\n"
    "          [--init plane|two-frame] [--trackers N] [--batch] [--lookahead] [--prerender] [--pageable] [--set SDVL.key value]\n"
    "          [--quiet] [--json] [--profile]\n";

// the frame of a --list file as an Image: a P6 is RGB, a P5 is gray or, with --raw-format, the bytes of that format (file_w = W x bytes per
// pixel of it); false if the file's width does not fit
bool WrapListFrame(const uint8_t *data, int file_w, int W, int H, int format, int raw_format, Image *img) {
  if (format == PIX_GRAY8 && raw_format) format = raw_format;
  const int row = W * PixelFormatBytes(format);
  if (file_w != (format == PIX_RGB8 ? W : row)) return false;
  *img = Image::Wrap(data, W, H, row, format);
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  int W = 640, H = 480, n_synth = 0;
  unsigned seed = 20260001;
  double cam4[4] = {517.3, 516.5, 318.6, 255.3}, dist[5] = {0, 0, 0, 0, 0}, plane[4] = {0, 0, 1, 2.0};
  std::string list, cfg, scene_name;
  bool mapper = false, bundle = false, two_frame = false, size_given = false, cam_given = false, dist_given = false;
  bool prerender = false, pageable = false, quiet = false, json = false, profile = false, batch = false, lookahead = false;
  int n_trackers = 1, raw_format = 0;
  bool depth = false, depth_mapping = false, plane_given = false, depth_bundle = false;
  double depth_bf = 0.0;
  std::string depth_list;
  double depth_scale = 0.0;
  bool stereo = false, stereo_mapping = false;
  double baseline = 0.0, disparity_sigma = 0.0;
  std::string right_list, rig_file;
  std::vector<std::pair<std::string, double>> sets;  // --set SDVL.key value, applied after the configuration file
  unsigned texture = SDVL_TEXTURE_PLANE_NOISE;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto need = [&](int k) { if (i + k >= argc) { std::cerr << "missing value after " << a << std::endl; std::exit(2); } };
    if (a == "--synthetic") { need(1); n_synth = std::atoi(argv[++i]); }
    else if (a == "--seed") { need(1); seed = static_cast<unsigned>(std::strtoul(argv[++i], nullptr, 10)); }
    else if (a == "--list") { need(1); list = argv[++i]; }
    else if (a == "--raw-format") { need(1); raw_format = RawFormatByName(argv[++i]); if (!raw_format) { std::cerr << "unknown --raw-format " << argv[i] << "\n" << kUsage; return 2; } }
    else if (a == "--help" || a == "-h") { std::cout << kUsage; return 0; }
    else if (a == "--config") { need(1); cfg = argv[++i]; }
    else if (a == "--size") { need(2); W = std::atoi(argv[++i]); H = std::atoi(argv[++i]); size_given = true; }
    else if (a == "--cam") { need(4); for (int k = 0; k < 4; k++) cam4[k] = std::atof(argv[++i]); cam_given = true; }
    else if (a == "--dist") { need(5); for (int k = 0; k < 5; k++) dist[k] = std::atof(argv[++i]); dist_given = true; }
    else if (a == "--plane") { need(4); for (int k = 0; k < 4; k++) plane[k] = std::atof(argv[++i]); plane_given = true; }
    else if (a == "--depth") depth = true;
    else if (a == "--depth-mapping") { depth_mapping = true; mapper = true; }
    else if (a == "--depth-bundle") { depth_bundle = true; bundle = true; mapper = true; }
    else if (a == "--depth-bf") { need(1); depth_bf = std::atof(argv[++i]); }
    else if (a == "--depth-list") { need(1); depth_list = argv[++i]; depth = true; }
    else if (a == "--depth-scale") { need(1); depth_scale = std::atof(argv[++i]); }
    else if (a == "--stereo") stereo = true;
    else if (a == "--baseline") { need(1); baseline = std::atof(argv[++i]); }
    else if (a == "--stereo-mapping") { stereo_mapping = true; mapper = true; }
    else if (a == "--disparity-sigma") { need(1); disparity_sigma = std::atof(argv[++i]); }
    else if (a == "--right-list") { need(1); right_list = argv[++i]; stereo = true; }
    else if (a == "--rig") { need(1); rig_file = argv[++i]; }
    else if (a == "--mapper") mapper = true;
    else if (a == "--bundle") { bundle = true; mapper = true; }  // local bundle adjustment of every new keyframe (SDVL::SetBundleAdjustment; implies --mapper)
    else if (a == "--init") { need(1); const std::string t = argv[++i]; if (t == "two-frame") { two_frame = true; mapper = true; } else if (t != "plane") { std::cerr << "unknown --init " << t << std::endl; return 2; } }
    else if (a == "--texture") { need(1); const std::string t = argv[++i]; if (t == "camera") texture = SDVL_TEXTURE_CAMERA; else if (t != "plane") { std::cerr << "unknown texture " << t << std::endl; return 2; } }
    else if (a == "--scene") { need(1); scene_name = argv[++i]; }
    else if (a == "--trackers") { need(1); n_trackers = std::max(1, std::atoi(argv[++i])); }
    else if (a == "--batch") batch = true;
    else if (a == "--lookahead") lookahead = true;
    else if (a == "--prerender") prerender = true;
    else if (a == "--pageable") pageable = true;
    else if (a == "--quiet") quiet = true;
    else if (a == "--json") json = true;
    else if (a == "--profile") profile = true;
    else if (a == "--set") { need(2); sets.emplace_back(argv[i + 1], std::atof(argv[i + 2])); i += 2; }
    else { std::cerr << "unknown argument " << a << std::endl; return 2; }
  }
  if ((n_synth > 0) == !list.empty()) { std::cerr << "give either --synthetic N or --list file" << std::endl; return 2; }
  if (raw_format && list.empty()) { std::cerr << "--raw-format says what the P5 files of a --list hold: give --list file" << std::endl; return 2; }
  sdvl_synth_scene scene_surfaces = {};  // --scene: n_surfaces and surfaces of the preset
  if (!scene_name.empty()) {
    if (n_synth <= 0) { std::cerr << "--scene renders the synthetic sequence: give --synthetic N" << std::endl; return 2; }
    if (sdvl_synth_scene_preset(scene_name.c_str(), &scene_surfaces) != 0) {
      std::cerr << "unknown --scene " << scene_name << " (one of: " << sdvl_synth_scene_preset_names() << ")" << std::endl;
      return 2;
    }
  }
  const bool use_scene = !scene_name.empty();
  if (depth_bundle && !depth) { std::cerr << "--depth-bundle takes its depths from the frames' depth images: give --depth or --depth-list too" << std::endl; return 2; }
  if (depth_mapping && !depth) { std::cerr << "--depth-mapping feeds the mapper from the frames' depth images: give --depth or --depth-list too" << std::endl; return 2; }
  if (depth) {
    if (depth_list.empty() && !use_scene) { std::cerr << "--depth tracks on the renderer's depth: give --synthetic N --scene NAME, or --depth-list FILE with --list" << std::endl; return 2; }
    if (!depth_list.empty() && (list.empty() || !(depth_scale > 0.0))) { std::cerr << "--depth-list goes with --list and --depth-scale S (metres per unit, above 0)" << std::endl; return 2; }
    if (batch || prerender || n_trackers > 1) { std::cerr << "--depth runs one camera on frames made inside the loop: not with --batch, --trackers or --prerender" << std::endl; return 2; }
    if (plane_given) std::cerr << "note: --plane is ignored, the keyframes' points are seeded from depth" << std::endl;
  }
  if (stereo_mapping && !stereo) { std::cerr << "--stereo-mapping feeds the mapper from the frames' right images: give --stereo or --right-list too" << std::endl; return 2; }
  if (!(disparity_sigma >= 0.0) || disparity_sigma > 1e300) { std::cerr << "--disparity-sigma X: pixels, not negative" << std::endl; return 2; }
  if (disparity_sigma != 0.0 && !stereo_mapping) { std::cerr << "--disparity-sigma is the noise of --stereo-mapping: give that too" << std::endl; return 2; }
  if (!rig_file.empty() && !stereo) { std::cerr << "--rig FILE describes the rig of --stereo / --right-list: give one of them too" << std::endl; return 2; }
  if (stereo) {  // what SDVL::SetStereoSeeding would throw, said before any device is touched
    if (right_list.empty() && !use_scene) { std::cerr << "--stereo tracks on the rendered right image: give --synthetic N --scene NAME, or --right-list FILE with --list" << std::endl; return 2; }
    if (!right_list.empty() && list.empty()) { std::cerr << "--right-list goes with --list" << std::endl; return 2; }
    if (rig_file.empty() && (!(baseline > 0.0) || baseline > 1e300)) { std::cerr << "--stereo and --right-list need --baseline B (metres, above 0)" << std::endl; return 2; }
    if (depth) { std::cerr << "--stereo and --depth / --depth-list both fill the frame's second image: give one" << std::endl; return 2; }
    if (two_frame) { std::cerr << "--stereo and --init two-frame answer the same question: give one" << std::endl; return 2; }
    if (batch || prerender || n_trackers > 1) { std::cerr << "--stereo runs one camera on frames made inside the loop: not with --batch, --trackers or --prerender" << std::endl; return 2; }
    if (plane_given) std::cerr << "note: --plane is ignored, the keyframes' points are seeded from the stereo pair" << std::endl;
  }

  // main.cc:60-75: configuration file, then the TUM overrides the reference's config_tum_f1.cfg carries
  Config &c = Config::GetInstance();
  c.SetParameter("SDVL.cell_size", 32); c.SetParameter("SDVL.max_matches", 200); c.SetParameter("SDVL.use_orb", 1);
  c.SetParameter("SDVL.fast_threshold", 10); c.SetParameter("SDVL.num_features", 1000); c.SetParameter("SDVL.min_avg_shift", 5);
  c.SetParameter("SDVL.max_keyframes", 1000); c.SetParameter("SDVL.lost_ratio", 0.7);
  if (!cfg.empty()) {
    if (!c.ReadParameters(cfg)) { std::cerr << "cannot read " << cfg << std::endl; return 2; }
    // the camera block of the file (main.cc:72: Camera() reads it) unless --size / --cam / --dist said otherwise
    const CameraParameters &cp = Config::GetCameraParameters();
    if (!size_given) { W = cp.width; H = cp.height; }
    if (!cam_given) { cam4[0] = cp.fx; cam4[1] = cp.fy; cam4[2] = cp.u0; cam4[3] = cp.v0; }
    if (!dist_given) { dist[0] = cp.d1; dist[1] = cp.d2; dist[2] = cp.d3; dist[3] = cp.d4; dist[4] = cp.d5; }
  }

  for (const auto &kv : sets)
    if (!c.SetParameter(kv.first, kv.second)) { std::cerr << "unknown parameter " << kv.first << std::endl; return 2; }

  std::vector<std::string> files;
  if (!list.empty()) {
    std::ifstream lf(list);
    for (std::string line; std::getline(lf, line);)
      if (!line.empty() && line[0] != '#') files.push_back(line);
    if (files.empty()) { std::cerr << "no frames in " << list << std::endl; return 2; }
  }
  std::vector<std::string> depth_files;
  if (!depth_list.empty()) {
    std::ifstream lf(depth_list);
    for (std::string line; std::getline(lf, line);)
      if (!line.empty() && line[0] != '#') depth_files.push_back(line);
    if (depth_files.size() != files.size()) { std::cerr << depth_list << " names " << depth_files.size() << " depth images for " << files.size() << " frames" << std::endl; return 2; }
  }
  std::vector<std::string> right_files;
  if (!right_list.empty()) {
    std::ifstream lf(right_list);
    for (std::string line; std::getline(lf, line);)
      if (!line.empty() && line[0] != '#') right_files.push_back(line);
    if (right_files.size() != files.size()) { std::cerr << right_list << " names " << right_files.size() << " right images for " << files.size() << " frames" << std::endl; return 2; }
  }
  if (stereo && rig_file.empty() && dist[0] != 0.0) {
    std::cerr << "--stereo takes rectified pairs: not with a lens (--dist, or the configuration file's Camera.d1); a rig as calibrated goes through --rig FILE" << std::endl;
    return 2;
  }
  // --rig: the plan of the rig (host code, no device); the tracker's camera is its rectified camera, the frames stay raw
  StereoRig rig;
  RectifiedPair pair;
  const bool rectify = !rig_file.empty();
  if (rectify) {
    std::string err;
    if (!ReadRig(rig_file, &rig, &err)) { std::cerr << err << std::endl; return 2; }
    for (int q = 0; q < 4; q++) rig.K1[q] = cam4[q];
    for (int q = 0; q < 5; q++) rig.D1[q] = dist[q];
    try {
      pair = RectifiedPair::Plan(rig, W, H);
    } catch (const std::exception &e) {
      std::cerr << "--rig " << rig_file << ": " << e.what() << std::endl;
      return 2;
    }
    baseline = pair.baseline;
    std::fprintf(stderr, "rectified camera: fx %.6f fy %.6f u0 %.6f v0 %.6f, baseline %.6f m\n", pair.camera().fx, pair.camera().fy, pair.camera().u0,
                 pair.camera().v0, pair.baseline);
  }
  const int n_frames = n_synth > 0 ? n_synth : static_cast<int>(files.size());

  const double tw[6] = {0.004, 0.002, 0.001, 0.0008, -0.0012, 0.0005};
  auto view_of = [&](int k) {  // T_k = Exp(k * xi), SURVEY §8d
    Vector6d xi;
    for (int q = 0; q < 6; q++) xi.v[q] = tw[q] * k;
    const SE3 T = SE3::Exp(xi);
    sdvl_synth_view v = {};
    v.fx = cam4[0]; v.fy = cam4[1]; v.u0 = cam4[2]; v.v0 = cam4[3];
    const M3 R = T.GetRotation();
    for (int q = 0; q < 9; q++) v.R[q] = R.m[q];
    const Vector3d t = T.GetTranslation();
    for (int q = 0; q < 3; q++) v.t[q] = t(q);
    for (int q = 0; q < 4; q++) v.plane[q] = plane[q];
    v.seed = seed;
    v.frame_id = static_cast<uint32_t>(k);
    v.texture = texture;
    for (int q = 0; q < 5; q++) v.dist[q] = dist[q];  // --dist: the frames are what a camera with that lens records (camera.UndistortImage undoes it)
    return v;
  };
  auto scene_of = [&](int k) {  // the same camera, pose, seeds and lens in front of the preset's surfaces
    const sdvl_synth_view v = view_of(k);
    sdvl_synth_scene sc = scene_surfaces;
    sc.fx = v.fx; sc.fy = v.fy; sc.u0 = v.u0; sc.v0 = v.v0;
    for (int q = 0; q < 9; q++) sc.R[q] = v.R[q];
    for (int q = 0; q < 3; q++) sc.t[q] = v.t[q];
    sc.seed = v.seed; sc.frame_id = v.frame_id; sc.texture = v.texture;
    for (int q = 0; q < 5; q++) sc.dist[q] = v.dist[q];
    return sc;
  };
  auto render_host = [&](int k, uint8_t *out) {
    if (use_scene) { const sdvl_synth_scene sc = scene_of(k); sdvl_synth_render_scene_host(&sc, W, H, out, W, nullptr, nullptr); }
    else { const sdvl_synth_view v = view_of(k); sdvl_synth_render_host(&v, W, H, out, W); }
  };

  try {
    const size_t frame_bytes = static_cast<size_t>(W) * H;
    // --prerender: all frames of the synthetic sequence, rendered by the device generator (the same bytes as the host one) into
    // page-locked (or, --pageable, plain) host memory before anything is timed
    uint8_t *pool = nullptr;
    bool pool_pinned = false;
    std::unique_ptr<Device> render_dev;
    if (prerender && n_synth > 0) {
      render_dev.reset(new Device(0));
      sdvl_ctx *rc = render_dev->ctx();
      if (pageable) {
        pool = static_cast<uint8_t *>(std::malloc(frame_bytes * n_frames));
        if (!pool) throw std::runtime_error("out of memory for the frame pool");
      } else {
        void *pp = nullptr;
        render_dev->Check(sdvl_host_alloc_pinned(rc, static_cast<int64_t>(frame_bytes * n_frames), &pp), "sdvl_host_alloc_pinned");
        pool = static_cast<uint8_t *>(pp);
        pool_pinned = true;
      }
      void *dbuf = nullptr;
      const int chunk = 32;
      render_dev->Check(sdvl_device_malloc(rc, static_cast<int64_t>(frame_bytes * chunk), &dbuf), "sdvl_device_malloc");
      for (int k0 = 0; k0 < n_frames; k0 += chunk) {
        const int n = std::min(chunk, n_frames - k0);
        if (use_scene) {
          std::vector<sdvl_synth_scene> scenes;
          for (int k = k0; k < k0 + n; k++) scenes.push_back(scene_of(k));
          render_dev->Check(sdvl_synth_render_scene(rc, n, scenes.data(), W, H, dbuf, static_cast<int64_t>(frame_bytes), nullptr, nullptr), "sdvl_synth_render_scene");
        } else {
          std::vector<sdvl_synth_view> views;
          for (int k = k0; k < k0 + n; k++) views.push_back(view_of(k));
          render_dev->Check(sdvl_synth_render(rc, n, views.data(), W, H, dbuf, static_cast<int64_t>(frame_bytes)), "sdvl_synth_render");
        }
        render_dev->Check(sdvl_device_download(rc, dbuf, static_cast<int64_t>(frame_bytes * n), pool + frame_bytes * k0), "sdvl_device_download");
      }
      render_dev->Check(sdvl_device_free(rc, dbuf), "sdvl_device_free");
    }

    struct PerTracker { double busy = 0.0; int tracked = 0; std::vector<float> ms; std::string err; PlaneMap::DepthStats depth; MapperMap::DepthMapStats depth_map; DepthBundleStats depth_bundle; };
    std::vector<PerTracker> per(n_trackers);
    std::atomic<int> ready{0};
    std::atomic<bool> go{false};
    std::chrono::steady_clock::time_point t_go;
    auto run_tracker = [&](int id) {
      PerTracker &me = per[id];
      try {
        Device dev(0);             // one per thread that enters the path; fails loudly without an MI355X
        Device::SetCurrent(&dev);
        Camera camera(W, H, rectify ? pair.camera().fx : cam4[0], rectify ? pair.camera().fy : cam4[1], rectify ? pair.camera().u0 : cam4[2],
                      rectify ? pair.camera().v0 : cam4[3]);
        if (!rectify) camera.SetDistortions(dist[0], dist[1], dist[2], dist[3], dist[4]);  // camera.cc:39-67 (--rig: the lenses are the pair's)
        std::unique_ptr<Map> map;
        if (mapper) map.reset(new MapperMap(Vector3d(plane[0], plane[1], plane[2]), plane[3], &camera));
        else map.reset(new PlaneMap(Vector3d(plane[0], plane[1], plane[2]), plane[3]));
        SDVL sdvl(&camera, map.get());
        if (two_frame) sdvl.SetTwoFrameInit(true);
        if (bundle) sdvl.SetBundleAdjustment(true);
        if (depth) sdvl.SetDepthSeeding(true);
        if (depth_mapping) sdvl.SetDepthMapping(true);
        if (depth_bundle) sdvl.SetDepthBundle(true, depth_bf);
        if (stereo) sdvl.SetStereoSeeding(true, baseline);
        if (rectify) sdvl.SetStereoRectification(pair);
        if (stereo_mapping) sdvl.SetStereoMapping(true, disparity_sigma);
        std::vector<uint8_t> right_px(stereo ? frame_bytes : 0);
        std::vector<float> depth_f32(depth && depth_list.empty() ? frame_bytes : 0);
        std::vector<uint16_t> depth_u16;
        std::vector<uint8_t> px(pool ? 0 : frame_bytes);
        me.ms.reserve(n_frames);
        Image ahead;
        bool ahead_valid = false;
        if (n_trackers > 1) {  // all cameras start together
          ready.fetch_add(1);
          while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
        }
        for (int k = 0; k < n_frames; k++) {
          uint8_t *data = px.data();
          int format = PIX_GRAY8, file_w = W;
          if (pool) {
            data = pool + frame_bytes * k;
          } else if (n_synth > 0 && depth) {  // the image and its registered depth (through the lens of --dist: both on the raw grid)
            const sdvl_synth_scene sc = scene_of(k);
            sdvl_synth_render_scene_host(&sc, W, H, px.data(), W, depth_f32.data(), nullptr);
          } else if (n_synth > 0) {
            render_host(k, px.data());
          } else {
            int w = 0, h = 0;
            if (!ReadPNM(files[k], &w, &h, &px, &format) || h != H) {
              me.err = "cannot read " + files[k] + " as a binary PGM / PPM of the configured size";
              return;
            }
            data = px.data();
            file_w = w;
          }
          Image img;  // a P6 frame, or a raw P5 frame: converted to gray on the device (video_source.cc:63)
          if (!WrapListFrame(data, file_w, W, H, format, raw_format, &img)) {
            me.err = "cannot read " + files[k] + " as a binary PGM / PPM of the configured size";
            return;
          }
          Image imgu;
          if (lookahead && pool && ahead_valid) {
            imgu = ahead;                                          // undistorted one iteration ago
          } else {
            camera.UndistortImage(img, &imgu);                      // main.cc:133
          }
          ahead_valid = false;
          if (lookahead && pool && k + 1 < n_frames) {              // the next frame is there already: undistort it now, name it
            Image nxt;
            nxt.data = pool + frame_bytes * (k + 1); nxt.cols = W; nxt.rows = H; nxt.step = W;
            camera.UndistortImage(nxt, &ahead);
            ahead_valid = true;
            if (k > 0) sdvl.SetNextImage(ahead);                   // (frame 0 is the bootstrap: no tracked step to queue behind)
          }
          if (k == 1 && profile) dev.Check(sdvl_ctx_timing_enable(dev.ctx(), 1), "sdvl_ctx_timing_enable");
          DepthImage dimg;
          if (depth && depth_list.empty()) {
            dimg = DepthImage::Wrap(depth_f32.data(), W, H, W * 4, DEPTH_F32, 1.0, false);
          } else if (depth) {
            int w = 0, h = 0;
            if (!ReadDepthPGM(depth_files[k], &w, &h, &depth_u16) || w != W || h != H) {
              me.err = "cannot read " + depth_files[k] + " as a 16-bit binary PGM of the configured size";
              return;
            }
            dimg = DepthImage::Wrap(depth_u16.data(), W, H, W * 2, DEPTH_U16, depth_scale, false);
          } else if (stereo) {
            if (right_list.empty()) {  // the same scene from the right camera: t_right = t_left - (B, 0, 0)
              sdvl_synth_scene sc = scene_of(k);
              if (rectify) {  // the right camera as calibrated: pose (R R_l, R t_l + T), its own intrinsics and lens
                const sdvl_synth_scene l = sc;
                for (int r = 0; r < 3; r++) {
                  for (int q = 0; q < 3; q++) sc.R[3 * r + q] = rig.R[3 * r] * l.R[q] + rig.R[3 * r + 1] * l.R[3 + q] + rig.R[3 * r + 2] * l.R[6 + q];
                  sc.t[r] = rig.R[3 * r] * l.t[0] + rig.R[3 * r + 1] * l.t[1] + rig.R[3 * r + 2] * l.t[2] + rig.T[r];
                }
                sc.fx = rig.K2[0]; sc.fy = rig.K2[1]; sc.u0 = rig.K2[2]; sc.v0 = rig.K2[3];
                for (int q = 0; q < 5; q++) sc.dist[q] = rig.D2[q];
              } else {
                sc.t[0] -= baseline;
              }
              sdvl_synth_render_scene_host(&sc, W, H, right_px.data(), W, nullptr, nullptr);
            } else {
              int w = 0, h = 0, fmt = PIX_GRAY8;
              if (!ReadPNM(right_files[k], &w, &h, &right_px, &fmt) || fmt != PIX_GRAY8 || w != W || h != H) {
                me.err = "cannot read " + right_files[k] + " as an 8-bit binary PGM of the configured size";
                return;
              }
            }
            dimg = DepthImage::Wrap(right_px.data(), W, H, W, DEPTH_RIGHT8, 1.0, false);
          }
          const auto t0 = std::chrono::steady_clock::now();
          sdvl.HandleFrame(imgu, dimg);                           // main.cc:136-138
          if (mapper) sdvl.Mapping();                             // sequential mode, main.cc:148-149
          const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          const FrameStats &st = sdvl.LastStats();
          if (k > 0) { me.busy += dt; me.tracked += st.quality != 2; me.ms.push_back(static_cast<float>(dt * 1e3)); }  // frame 0 is the bootstrap keyframe
          if (!quiet && id == 0)
            std::printf("%d %d %d %d %d %d  %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", k, st.state, st.quality, st.matches, st.attempts, st.inliers,
                        st.pose[0], st.pose[1], st.pose[2], st.pose[3], st.pose[4], st.pose[5], st.pose[6]);
        }
        if (depth || stereo) me.depth = dynamic_cast<PlaneMap *>(map.get())->GetDepthStats();
        if (depth_mapping || stereo_mapping) me.depth_map = dynamic_cast<MapperMap *>(map.get())->GetDepthMapStats();
        if (depth_bundle) me.depth_bundle = dynamic_cast<MapperMap *>(map.get())->GetDepthBundleStats();
        if (profile && id == 0) {
          char names[32][32];
          double ms[32];
          int64_t launches[32];
          int n = 0;
          dev.Check(sdvl_ctx_timing_get(dev.ctx(), 32, names, ms, launches, &n), "sdvl_ctx_timing_get");
          const int nf = std::max(1, n_frames - 1);
          double sum = 0.0;
          for (int q = 0; q < n; q++) sum += ms[q];
          std::fprintf(stderr, "kernel dispatch time per tracked frame (HIP events on the tracker's stream, %d frames): total %.1f us\n", nf, sum / nf * 1e3);
          for (int q = 0; q < n; q++)
            std::fprintf(stderr, "  %-24s %8.1f us/frame  %6.2f launches/frame  %7.1f us/launch\n", names[q], ms[q] / nf * 1e3,
                         static_cast<double>(launches[q]) / nf, launches[q] ? ms[q] / launches[q] * 1e3 : 0.0);
          if (const StageTimes *stt = sdvl.HandleFrameStageTimes()) {
            static const char *stage_names[] = {"upload_pyr", "fast", "select", "corners_orb", "prelude", "image_align", "prepare", "search", "finish", "pose",
                                                "mapping", "epilogue", "mapper", "total"};
            std::fprintf(stderr, "host stages per HandleFrame (wall, %ld calls):\n", stt->steps);
            for (int q = 0; q <= ST_TOTAL; q++)
              if (stt->t[q] > 0) std::fprintf(stderr, "  %-12s %8.1f us\n", stage_names[q], stt->t[q] / std::max(1L, stt->steps) * 1e6);
          }
        }
      } catch (const std::exception &e) {
        me.err = e.what();
      }
    };
    // --batch: the N cameras are frames of ONE SDVLBatch::HandleFrames call (one thread, one stream, one launch per kernel for all N)
    auto run_batch = [&]() {
      PerTracker &me = per[0];
      try {
        Device dev(0);
        Device::SetCurrent(&dev);
        Camera camera(W, H, cam4[0], cam4[1], cam4[2], cam4[3]);
        camera.SetDistortions(dist[0], dist[1], dist[2], dist[3], dist[4]);
        std::vector<std::unique_ptr<Map>> maps;
        std::vector<std::unique_ptr<SDVL>> trackers;
        std::vector<SDVL *> raw;
        for (int i = 0; i < n_trackers; i++) {
          if (mapper) maps.emplace_back(new MapperMap(Vector3d(plane[0], plane[1], plane[2]), plane[3], &camera));
          else maps.emplace_back(new PlaneMap(Vector3d(plane[0], plane[1], plane[2]), plane[3]));
          trackers.emplace_back(new SDVL(&camera, maps.back().get()));
          if (two_frame) trackers.back()->SetTwoFrameInit(true);
          if (bundle) trackers.back()->SetBundleAdjustment(true);
          raw.push_back(trackers.back().get());
        }
        {
          SDVLBatch b(&dev, raw, 1);
          std::vector<FrameStats> st(n_trackers);
          std::vector<uint8_t> px(pool ? 0 : frame_bytes);
          for (int k = 0; k < n_frames; k++) {
            uint8_t *data = px.data();
            if (pool) data = pool + frame_bytes * k;
            else if (n_synth > 0) render_host(k, px.data());
            int format = PIX_GRAY8, file_w = W;
            if (!pool && n_synth == 0) { int w = 0, h = 0; if (!ReadPNM(files[k], &w, &h, &px, &format) || h != H) { me.err = "cannot read " + files[k]; return; } data = px.data(); file_w = w; }
            Image img;
            if (!WrapListFrame(data, file_w, W, H, format, raw_format, &img)) { me.err = "cannot read " + files[k]; return; }
            std::vector<Image> imgs(n_trackers);
            for (int i = 0; i < n_trackers; i++) camera.UndistortImage(img, &imgs[i]);  // every camera its own frame in HBM (main.cc:133, outside the window)
            const auto t0 = std::chrono::steady_clock::now();
            b.HandleFrames(imgs, st.data());
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (k > 0) {
              me.busy += dt;
              for (int i = 0; i < n_trackers; i++) me.tracked += st[i].quality != 2;
              me.ms.push_back(static_cast<float>(dt * 1e3));
            }
            if (!quiet)
              std::printf("%d %d %d %d %d %d  %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", k, st[0].state, st[0].quality, st[0].matches, st[0].attempts, st[0].inliers,
                          st[0].pose[0], st[0].pose[1], st[0].pose[2], st[0].pose[3], st[0].pose[4], st[0].pose[5], st[0].pose[6]);
          }
        }
        trackers.clear();
        maps.clear();
      } catch (const std::exception &e) {
        me.err = e.what();
      }
    };
    double wall = 0.0;
    if (batch) {
      const auto w0 = std::chrono::steady_clock::now();
      run_batch();
      wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    } else if (n_trackers == 1) {
      const auto w0 = std::chrono::steady_clock::now();
      run_tracker(0);
      wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    } else {
      std::vector<std::thread> th;
      for (int i = 0; i < n_trackers; i++) th.emplace_back(run_tracker, i);
      while (ready.load() < n_trackers) {
        bool failed = false;
        for (const PerTracker &p : per) failed = failed || !p.err.empty();
        if (failed) break;
        std::this_thread::yield();
      }
      const auto w0 = std::chrono::steady_clock::now();
      go.store(true, std::memory_order_release);
      for (std::thread &t : th) t.join();
      wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    }
    for (const PerTracker &p : per)
      if (!p.err.empty()) { std::cerr << "track_sequence: " << p.err << std::endl; return 1; }
    if (pool) {
      if (pool_pinned) render_dev->Check(sdvl_host_free_pinned(render_dev->ctx(), pool), "sdvl_host_free_pinned");
      else std::free(pool);
    }
    int tracked = 0;
    double busy_max = 0.0, busy_sum = 0.0;
    std::vector<float> all_ms;
    for (const PerTracker &p : per) {
      tracked += p.tracked;
      busy_max = std::max(busy_max, p.busy);
      busy_sum += p.busy;
      all_ms.insert(all_ms.end(), p.ms.begin(), p.ms.end());
    }
    std::sort(all_ms.begin(), all_ms.end());
    const auto pct = [&](double q) { return all_ms.empty() ? 0.0 : static_cast<double>(all_ms[std::min(all_ms.size() - 1, static_cast<size_t>(q * all_ms.size()))]); };
    // one camera: tracked frames over the summed HandleFrame time (the window of main.cc:136-138).  N cameras: every camera's own rate is
    // its tracked frames over ITS summed HandleFrame time; the job's rate is all tracked frames over the slowest camera's summed time
    const double total = busy_max > 0 ? tracked / busy_max : 0.0;
    const double per_camera = batch ? total / n_trackers : (busy_sum > 0 ? tracked / busy_sum : 0.0);
    std::fprintf(stderr, "%d tracked frames in %.3f s of HandleFrame = %.1f tracked frames/s (%d sequence(s), one stream each; per camera %.1f)\n", tracked,
                 busy_max, total, n_trackers, per_camera);
    if (depth) {
      const PlaneMap::DepthStats &d = per[0].depth;
      std::fprintf(stderr, "depth seeding: %ld keyframes, %ld seeds; corners OK %ld HOLE %ld FEW %ld EDGE %ld OUTSIDE %ld; %ld frames without depth\n", d.keyframes, d.seeds,
                   d.by_status[0], d.by_status[1], d.by_status[2], d.by_status[3], d.by_status[4], d.no_depth);
    }
    if (stereo) {
      const PlaneMap::DepthStats &d = per[0].depth;
      std::fprintf(stderr, "stereo seeding: %ld keyframes, %ld seeds; corners OK %ld NOMATCH %ld AMBIGUOUS %ld EDGE %ld OUTSIDE %ld; %ld frames without a right image\n",
                   d.keyframes, d.seeds, d.by_status[0], d.by_status[1], d.by_status[2], d.by_status[3], d.by_status[4], d.no_depth);
    }
    char depth_map_json[256] = "";
    if (depth_mapping) {
      const MapperMap::DepthMapStats &d = per[0].depth_map;
      std::fprintf(stderr, "depth mapping: %ld measured updates, fallen back HOLE %ld FEW %ld EDGE %ld OUTSIDE %ld; %ld keyframes looked up, corners fixed %ld matched + %ld unmatched, %ld linked\n",
                   d.measured, d.fallback[0], d.fallback[1], d.fallback[2], d.fallback[3], d.keyframes, d.fixed_matched, d.fixed_unmatched, d.linked);
      std::snprintf(depth_map_json, sizeof(depth_map_json),
                    ", \"depth_mapping\": {\"measured\": %ld, \"hole\": %ld, \"few\": %ld, \"edge\": %ld, \"outside\": %ld, \"keyframes\": %ld, \"fixed_matched\": %ld, "
                    "\"fixed_unmatched\": %ld, \"linked\": %ld}",
                    d.measured, d.fallback[0], d.fallback[1], d.fallback[2], d.fallback[3], d.keyframes, d.fixed_matched, d.fixed_unmatched, d.linked);
    }
    if (stereo_mapping) {
      const MapperMap::DepthMapStats &d = per[0].depth_map;
      std::fprintf(stderr, "stereo mapping: %ld measured updates, fallen back NOMATCH %ld AMBIGUOUS %ld EDGE %ld OUTSIDE %ld; %ld keyframes matched, corners fixed %ld matched + %ld unmatched, %ld linked\n",
                   d.measured, d.fallback[0], d.fallback[1], d.fallback[2], d.fallback[3], d.keyframes, d.fixed_matched, d.fixed_unmatched, d.linked);
      std::snprintf(depth_map_json, sizeof(depth_map_json),
                    ", \"stereo_mapping\": {\"measured\": %ld, \"nomatch\": %ld, \"ambiguous\": %ld, \"edge\": %ld, \"outside\": %ld, \"keyframes\": %ld, "
                    "\"fixed_matched\": %ld, \"fixed_unmatched\": %ld, \"linked\": %ld}",
                    d.measured, d.fallback[0], d.fallback[1], d.fallback[2], d.fallback[3], d.keyframes, d.fixed_matched, d.fixed_unmatched, d.linked);
    }
    char depth_bundle_json[320] = "";
    if (depth_bundle) {
      const DepthBundleStats &d = per[0].depth_bundle;
      std::fprintf(stderr, "depth edges: lookups OK %ld HOLE %ld FEW %ld EDGE %ld OUTSIDE %ld, %ld observations with a depth; all windows: %ld edges, %ld with a depth, "
                   "%ld of those on level 1\n", d.lookups[0], d.lookups[1], d.lookups[2], d.lookups[3], d.lookups[4], d.stored, d.total_edges, d.total_depth_edges,
                   d.total_depth_level1);
      std::snprintf(depth_bundle_json, sizeof(depth_bundle_json),
                    ", \"depth_bundle\": {\"ok\": %ld, \"hole\": %ld, \"few\": %ld, \"edge\": %ld, \"outside\": %ld, \"stored\": %ld, \"edges\": %ld, "
                    "\"depth_edges\": %ld, \"depth_level1\": %ld}",
                    d.lookups[0], d.lookups[1], d.lookups[2], d.lookups[3], d.lookups[4], d.stored, d.total_edges, d.total_depth_edges, d.total_depth_level1);
    }
    if (json)
      std::printf("{\"trackers\": %d, \"frames\": %d, \"tracked\": %d, \"frames_per_s\": %.2f, \"frames_per_s_per_camera\": %.2f, \"ms_per_frame_p50\": %.4f, "
                  "\"ms_per_frame_p95\": %.4f, \"ms_per_frame_max\": %.4f, \"wall_s\": %.3f, \"input\": \"%s\", \"texture\": \"%s\", \"width\": %d, \"height\": %d, "
                  "\"mapper\": %s, \"api\": \"%s\"%s%s}\n",
                  n_trackers, n_frames, tracked, total, per_camera, pct(0.5), pct(0.95), all_ms.empty() ? 0.0 : static_cast<double>(all_ms.back()), wall,
                  pool ? (pool_pinned ? "page-locked host memory" : "pageable host memory") : "host memory of the loop (pageable)",
                  texture == SDVL_TEXTURE_CAMERA ? "camera" : "plane", W, H, mapper ? "true" : "false",
                  batch ? "sdvl::SDVLBatch::HandleFrames, one call per frame for all cameras (one thread, one stream)"
                  : lookahead ? "SDVL::SetNextImage + SDVL::HandleFrame per frame (the next frame of the sequence named one call ahead)"
                        : "SDVL::HandleFrame per frame and camera (host/track_sequence.cc, the loop of main.cc:126-159; one thread and stream per camera)",
                  depth_map_json, depth_bundle_json);
  } catch (const std::exception &e) {
    std::cerr << "track_sequence: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
