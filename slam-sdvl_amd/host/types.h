// types.h — the small Eigen / OpenCV look-alikes the SDVL API surface is written in (frame.h:45-139,
// feature.h:42-94, sdvl.h:49-69).  Only what the tracking front-end touches: fixed-size vectors with Eigen's
// operator() access, and Image = the cv::Mat (CV_8UC1) subset {data, cols, rows, step} plus a binding to the
// HBM-resident pyramid level it mirrors.  With real Eigen/OpenCV available a maintainer maps these 1:1
// (INTEGRATION.md).
#ifndef SDVL_HOST_TYPES_H_
#define SDVL_HOST_TYPES_H_

#include <stdint.h>

#include <memory>
#include <stdexcept>
#include <vector>

#include "../../include/sdvl_hip.h"

// Real Eigen / OpenCV, when the build has them (this image has neither): the look-alikes below then convert to and from the real
// types, so callers written against the reference's headers (sdvl.cc, map.cc, ui/: cv::Mat frames in, Eigen vectors out) pass and
// receive their own types — SDVL::HandleFrame(const cv::Mat&) (sdvl.h:62), Frame(..., const cv::Mat&, ...) (frame.h:45),
// Feature::GetPosition() -> Eigen::Vector2d (feature.h:66).  -DSDVL_NO_THIRD_PARTY_TYPES keeps the build free of both.
#if !defined(SDVL_NO_THIRD_PARTY_TYPES) && defined(__has_include)
#if __has_include(<Eigen/Dense>)
#include <Eigen/Dense>
#define SDVL_HAVE_EIGEN 1
#endif
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define SDVL_HAVE_OPENCV 1
#endif
#endif

struct sdvl_frame;

namespace sdvl {

typedef unsigned char uchar;

template <typename T, int N>
struct Vec {
  T v[N];
  Vec() { for (int i = 0; i < N; i++) v[i] = T(); }
  Vec(T a, T b) { static_assert(N == 2, "size"); v[0] = a; v[1] = b; }
  Vec(T a, T b, T c) { static_assert(N == 3, "size"); v[0] = a; v[1] = b; v[2] = c; }
  T &operator()(int i) { return v[i]; }
  const T &operator()(int i) const { return v[i]; }
  T &operator[](int i) { return v[i]; }
  const T &operator[](int i) const { return v[i]; }
  T x() const { return v[0]; }
  T y() const { return v[1]; }
#ifdef SDVL_HAVE_EIGEN
  // Eigen::Matrix<T, N, 1> in and out (Vector2d / Vector3d / Vector3i / Vector6d of the reference's signatures)
  Vec(const Eigen::Matrix<T, N, 1> &e) { for (int i = 0; i < N; i++) v[i] = e(i); }
  operator Eigen::Matrix<T, N, 1>() const {
    Eigen::Matrix<T, N, 1> e;
    for (int i = 0; i < N; i++) e(i) = v[i];
    return e;
  }
#endif
};
typedef Vec<double, 2> Vector2d;
typedef Vec<double, 3> Vector3d;
typedef Vec<int, 2> Vector2i;
typedef Vec<int, 3> Vector3i;
typedef Vec<double, 6> Vector6d;

// cv::Mat (CV_8UC1) subset.  `data` is a host mirror (may be null until HostData() is called on the owning
// Frame); dev/level bind the image to an HBM-resident pyramid level.
#ifndef SDVL_HAVE_OPENCV
enum { CV_8UC1 = 0 };  // the only cv::Mat type the tracking front-end sees (frame.cc:38-41 converts to grey)
#endif

// Pixel layout of an Image (= enum sdvl_pixel_format of include/sdvl_hip.h).  A colour image is a RAW camera frame: the Frame built from it
// takes cv::cvtColor(frame, img, CV_*2GRAY) (video_source.cc:63) as its image, converted on the device inside the upload.
// From 16 on (= enum sdvl_raw_format): RAW camera formats, converted the same way.  A Bayer mosaic is named by the 2x2 tile at its top-left
// corner; YUYV / UYVY and the 16-bit grays (little-endian, 10 / 12 / 16 significant bits) take two bytes per pixel.
enum PixelFormat {
  PIX_GRAY8 = 0, PIX_RGB8 = 1, PIX_BGR8 = 2, PIX_RGBA8 = 3, PIX_BGRA8 = 4,
  PIX_BAYER_RGGB8 = 16, PIX_BAYER_GRBG8 = 17, PIX_BAYER_GBRG8 = 18, PIX_BAYER_BGGR8 = 19,
  PIX_YUYV8 = 20, PIX_UYVY8 = 21, PIX_GRAY10_16 = 22, PIX_GRAY12_16 = 23, PIX_GRAY16 = 24
};
// the cv::Mat type codes of 8-bit 3- and 4-channel images (CV_8UC3, CV_8UC4) and of 16-bit gray (CV_16UC1)
enum { SDVL_CV_8UC3 = 16, SDVL_CV_8UC4 = 24, SDVL_CV_16UC1 = 2 };
// bytes per pixel of a PixelFormat, 0 for a value that is none
inline int PixelFormatBytes(int format) {
  return format == PIX_GRAY8 ? 1 : (format == PIX_RGB8 || format == PIX_BGR8) ? 3 : (format == PIX_RGBA8 || format == PIX_BGRA8) ? 4
       : (format >= PIX_BAYER_RGGB8 && format <= PIX_BAYER_BGGR8) ? 1 : (format >= PIX_YUYV8 && format <= PIX_GRAY16) ? 2 : 0;
}

struct Image {
  const uint8_t *data = nullptr;
  int cols = 0, rows = 0, step = 0;  // step: bytes between rows
  // colour images default to the REFERENCE's order: the R weight on byte 0 (CV_RGB2GRAY, video_source.cc:63 — applied there to the BGR
  // bytes of cv::VideoCapture, so this reproduces main.cc bit for bit); bgr() picks CV_BGR2GRAY, the luma of the true colours of BGR bytes
  int format = PIX_GRAY8;
  Image() {}
  // cv::Mat(rows, cols, type, data, step): a header over caller-owned pixels; type CV_8UC3 / CV_8UC4 = a colour frame
  Image(int rows_, int cols_, int type, const void *pixels, size_t step_ = 0)
      : data(static_cast<const uint8_t *>(pixels)), cols(cols_), rows(rows_),
        format(type == SDVL_CV_8UC3 ? PIX_RGB8 : type == SDVL_CV_8UC4 ? PIX_RGBA8 : type == SDVL_CV_16UC1 ? PIX_GRAY16 : PIX_GRAY8) {
    step = step_ ? static_cast<int>(step_) : cols_ * bytes_per_pixel();
  }
  // colour channels of a pixel (raw formats: 1), and the bytes it takes in a row
  int channels() const { return (format == PIX_RGB8 || format == PIX_BGR8) ? 3 : (format == PIX_RGBA8 || format == PIX_BGRA8) ? 4 : 1; }
  int bytes_per_pixel() const { return PixelFormatBytes(format); }
  bool color() const { return format != PIX_GRAY8; }
  // the same pixels, converted as CV_BGR2GRAY (the R weight on byte 2); a gray image stays as it is
  Image bgr() const {
    Image r = *this;
    if (format == PIX_RGB8) r.format = PIX_BGR8;
    if (format == PIX_RGBA8) r.format = PIX_BGRA8;
    return r;
  }
  // the same bytes as a Bayer mosaic of `order` (PIX_BAYER_*: the tile at the top-left corner), for a one-byte image (what a camera SDK
  // or a PGM file hands over as "gray"); any other image, or a value that is no Bayer order, stays as it is
  Image bayer(int order) const {
    Image r = *this;
    if (bytes_per_pixel() == 1 && order >= PIX_BAYER_RGGB8 && order <= PIX_BAYER_BGGR8) r.format = order;
    return r;
  }
  sdvl_frame *dev = nullptr;
  int level = 0;
  std::shared_ptr<std::vector<uint8_t>> owner;  // keeps a host copy alive (cv::Mat ref-count analogue)
  bool empty() const { return cols == 0 || rows == 0; }
  Image clone() const {
    Image r = *this;
    if (data) {
      const int row = cols * bytes_per_pixel();
      r.owner = std::make_shared<std::vector<uint8_t>>(static_cast<size_t>(row) * rows);
      for (int y = 0; y < rows; y++)
        for (int x = 0; x < row; x++) (*r.owner)[static_cast<size_t>(y) * row + x] = data[static_cast<size_t>(y) * step + x];
      r.data = r.owner->data();
      r.step = row;
    }
    return r;
  }
#ifdef SDVL_HAVE_OPENCV
  // a cv::Mat frame as the reference passes it (CV_8UC1, main.cc:128-138): a header over its pixels, the Mat kept alive.  A 3- or
  // 4-channel Mat (type 16 = CV_8UC3, 24 = CV_8UC4) is a colour frame in the reference's order (see `format`).
  Image(const cv::Mat &m) {
    const int t = m.empty() ? -1 : m.type();
    if (t == CV_8UC1 || t == SDVL_CV_8UC3 || t == SDVL_CV_8UC4 || t == SDVL_CV_16UC1) {
      format = t == SDVL_CV_8UC3 ? PIX_RGB8 : t == SDVL_CV_8UC4 ? PIX_RGBA8 : t == SDVL_CV_16UC1 ? PIX_GRAY16 : PIX_GRAY8;
      auto keep = std::make_shared<cv::Mat>(m);
      mat_owner = keep;
      data = keep->data;
      cols = keep->cols;
      rows = keep->rows;
      step = static_cast<int>(keep->step);
    }
  }
  // the host mirror as a cv::Mat header (GetPyramid() users: homography_init.cc:196, ui/drawimage.cc); empty while only the HBM copy exists
  operator cv::Mat() const {
    const int t = bytes_per_pixel() == 2 ? SDVL_CV_16UC1 : channels() == 1 ? CV_8UC1 : channels() == 3 ? SDVL_CV_8UC3 : SDVL_CV_8UC4;
    return data ? cv::Mat(rows, cols, t, const_cast<uint8_t *>(data), static_cast<size_t>(step)) : cv::Mat();
  }
  std::shared_ptr<void> mat_owner;
#endif
  static Image Wrap(const uint8_t *p, int w, int h, int stride) {
    Image r;
    r.data = p; r.cols = w; r.rows = h; r.step = stride;
    return r;
  }
  // an image that already lives in HBM (device pointer), e.g. a decoded camera frame
  const void *dev_src = nullptr;
  std::shared_ptr<void> dev_owner;  // keeps an HBM image produced by this layer alive (Camera::UndistortImage)
  bool borrow = false;  // the HBM image outlives every Frame built from it: alias it instead of copying
  // borrow + transient: the HBM image stays valid for the step that tracks it only (a slot of an input ring): the Frame aliases it
  // and takes a copy if it becomes a keyframe (Frame::OwnImages) — one frame in five in S-A, the other four never copy
  bool transient = false;
  // (an addition) a RAW camera image: the Frame built from it takes Camera::UndistortImage(image) (camera.cc:100-105, main.cc:133) as its
  // level 0 — the undistortion fused into the frame's upload, for callers that hand whole batches of camera frames to SDVLBatch
  bool raw = false;
  static Image WrapDevice(const void *dev_ptr, int w, int h, int stride, bool borrow_storage = false, bool transient_storage = false) {
    Image r;
    r.dev_src = dev_ptr; r.cols = w; r.rows = h; r.step = stride; r.borrow = borrow_storage; r.transient = borrow_storage && transient_storage;
    return r;
  }
  // the same with a pixel format: a colour image (host or HBM, row stride in bytes) is converted into the Frame's own level 0 — never
  // aliased, so borrow / transient do not apply to it
  static Image Wrap(const uint8_t *p, int w, int h, int stride, int pixel_format) {
    Image r = Wrap(p, w, h, stride);
    r.format = pixel_format;
    return r;
  }
  static Image WrapDeviceFormat(const void *dev_ptr, int w, int h, int stride, int pixel_format, bool borrow_storage) {
    Image r = WrapDevice(dev_ptr, w, h, stride, borrow_storage);
    r.format = pixel_format;
    return r;
  }
};

// (an addition) A depth image REGISTERED to the camera image as delivered (the raw pixel grid): a header over caller-owned samples, host or
// HBM.  DEPTH_F32: metres; DEPTH_U16: units of `scale` metres (TUM 1 / 5000, millimetres 0.001) — enum sdvl_depth_format of
// include/sdvl_hip.h.  Read only while a keyframe's points are seeded (sdvl_depth_seed), never copied or kept.  Empty means none.
// DEPTH_RIGHT8 is no depth image: the rectified right image of a stereo pair travels in the same slot (SDVL::SetStereoSeeding) — 8-bit
// gray, dense or strided rows, `scale` unused, host or HBM
enum DepthFormat { DEPTH_F32 = 0, DEPTH_U16 = 1, DEPTH_RIGHT8 = 2 };
struct DepthImage {
  const void *data = nullptr;
  int cols = 0, rows = 0, step = 0;  // step: bytes between rows
  int format = DEPTH_F32;
  double scale = 1.0;
  bool on_device = false;
  bool empty() const { return !data || cols == 0 || rows == 0; }
  static DepthImage Wrap(const void *p, int w, int h, int stride, int depth_format, double metres_per_unit, bool device) {
    DepthImage r;
    r.data = p; r.cols = w; r.rows = h; r.step = stride; r.format = depth_format; r.scale = metres_per_unit; r.on_device = device;
    return r;
  }
};

// (an addition) A stereo rig as calibrated: K_i = fx fy u0 v0, D_i = k1 k2 p1 p2 k3 (Camera.d1..d5), R (row-major) and T with
// X_right = R X_left + T — OpenCV's convention; the ideal rig is R = I, T = (-baseline, 0, 0).
struct StereoRig {
  double K1[4] = {0, 0, 0, 0}, D1[5] = {0, 0, 0, 0, 0};
  double K2[4] = {0, 0, 0, 0}, D2[5] = {0, 0, 0, 0, 0};
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0};
};

// (an addition) The plan of a rig's rectification (sdvl_stereo_rectify_plan, include/sdvl_hip.h): what each camera's map is built from,
// the one rectified pinhole camera of both images and the baseline.  SDVL::SetStereoRectification takes it.
struct RectifiedPair {
  sdvl_rectification left = {}, right = {};
  double baseline = 0.0;
  int width = 0, height = 0;
  const sdvl_camera &camera() const { return left.rect; }  // fx fy u0 v0 (and the size) of the rectified images
  // throws std::invalid_argument with the plan's message for a rig it refuses; `intrinsics`: the rectified camera's, instead of the plan's
  static RectifiedPair Plan(const StereoRig &rig, int width, int height, const sdvl_camera *intrinsics = nullptr) {
    sdvl_stereo_rig r;
    r.left = sdvl_camera{static_cast<double>(width), static_cast<double>(height), rig.K1[0], rig.K1[1], rig.K1[2], rig.K1[3]};
    r.right = sdvl_camera{static_cast<double>(width), static_cast<double>(height), rig.K2[0], rig.K2[1], rig.K2[2], rig.K2[3]};
    for (int i = 0; i < 5; i++) { r.left_dist.d[i] = rig.D1[i]; r.right_dist.d[i] = rig.D2[i]; }
    for (int i = 0; i < 9; i++) r.R[i] = rig.R[i];
    for (int i = 0; i < 3; i++) r.T[i] = rig.T[i];
    sdvl_stereo_rectified out;
    const int rc = sdvl_stereo_rectify_plan(&r, width, height, intrinsics, &out);
    if (rc != 0) throw std::invalid_argument(sdvl_stereo_rectify_plan_message(rc));
    RectifiedPair p;
    p.left = out.left; p.right = out.right; p.baseline = out.baseline; p.width = width; p.height = height;
    return p;
  }
};

}  // namespace sdvl

#endif  // SDVL_HOST_TYPES_H_
