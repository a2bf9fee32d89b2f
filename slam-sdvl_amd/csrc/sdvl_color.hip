// sdvl_color.hip — K0 input stage, first half: cv::cvtColor(frame, img, CV_RGB2GRAY) on every camera frame (video_source.cc:63), on the
// device, fused into the frames' upload.  The second half, Camera::UndistortImage (main.cc:133), follows it unchanged (sdvl_undistort.hip):
// undistort(gray(raw)), the order of main.cc:128-137.
//
// The arithmetic is OpenCV's 8-bit fixed-point luma (restated from OpenCV's source, not from the reference tree: unpinned there, like
// cv::pyrDown and cv::FAST):  Y = (c0 w0 + c1 w1 + c2 w2 + 2^13) >> 14  with R 4899, G 9617, B 1868 (sum 2^14: gray maps to itself).
// CV_RGB2GRAY weights byte 0 with R, CV_BGR2GRAY byte 2; 4-channel pixels use the same weights and ignore byte 3.  The order is uniform
// per launch (two kernel arguments), never decided per pixel.
//
// to_gray_kernel reads the colour bytes where they lie — pinned host memory through its device address, or HBM — so colour crosses the
// link once and no colour copy is staged in HBM (pageable sources are: hipMemcpy2DAsync into the context's scratch first).  Dense and
// aligned images: a lane converts 16 pixels from three (RGB) or four (RGBA) dwordx4 loads and writes them with ONE dwordx4 store (byte
// stores cost up to ~12x per byte); padded rows whose starts stay 16-byte aligned take the same path row by row; anything else (odd
// strides, odd widths, unaligned sources) goes row by row with byte accesses.  HBM-bound: (C + 1) W H bytes per frame.
//
// RAW camera formats (enum sdvl_raw_format) take the same route to the same gray.  Their arithmetic is stated in tests/raw_restatement.py,
// which is the specification (exact integers; not pinned to OpenCV):
//   YUYV / UYVY and 16-bit gray (wide_gray_kernel): two bytes per pixel, so a lane turns TWO dwordx4 loads into one dwordx4 store.  YUV
//     4:2:2 selects the Y byte of each pair (nothing is multiplied); 16-bit gray adds half and shifts by depth - 8, saturating at 255.  The
//     byte to select and the shift are kernel arguments.  Every source byte is read once: pinned host memory is read in place, as RGB is.
//   Bayer (bayer_gray_kernel): bilinear demosaic times 4 and to_gray's weights in one step.  With Hh / Vv the sums of the two row / column
//     neighbours and D the sum of the four diagonal ones, every site's luma is (a m + b Hh + c Vv + d D + 2^15) >> 16, where (a, b, c, d)
//     depends on the site's position in the 2x2 tile alone: a 4 x 4 table made on the host from the position of the red site, a kernel
//     argument.  A lane makes a 16 x 2 block aligned to the tile, so the table's row is a compile-time index at each of its 32 pixels.  It
//     takes four dwordx4 row loads (rows r - 1 .. r + 2) and eight byte loads for the columns left and right of the block; reflection (-1 ->
//     1, n -> n - 2) applies to the indices at the image's four edges only.  Rows shared by vertically adjacent blocks, and the halo bytes,
//     are left to the vector cache and L2: an image row is at most 16 KiB, the lanes that share it run in the same or the next workgroup,
//     and a strip staged in LDS would add a barrier and a second pass over the same bytes to save loads that already hit.  Because every
//     source row is read three times, a Bayer source in HOST memory, pinned or pageable, is always staged in the context's scratch
//     (one copy per run of tight images that follow each other, else one per image) and converted from HBM.  Widths that are no multiple of 16 and unaligned images go pixel by pixel.
//   HBM traffic: (bpp + 1) W H bytes per frame.
#include <vector>

#include "sdvl_internal.h"

namespace {

enum { kScalar = 0, kRows16 = 1, kFlat16 = 2 };

struct GrayJob {
  const uint8_t *src;  // device-visible address of the colour image
  uint8_t *dst;        // gray output
  long long sstride;   // bytes between source rows (per job: a staged copy is tight, a source read in place keeps the caller's pitch)
  int mode;            // kScalar / kRows16 / kFlat16
  int pad_;
};

constexpr int kW1 = 9617;          // G
constexpr int kWR = 4899, kWB = 1868;
constexpr int kMaxChunks = 1024;   // workgroups per image at most (a 4096 x 4096 image: four 16-pixel units per lane)
constexpr int kMaxSide = 16384;

int channels_of(int format) {
  switch (format) {
    case SDVL_GRAY8: return 1;
    case SDVL_RGB8: case SDVL_BGR8: return 3;
    case SDVL_RGBA8: case SDVL_BGRA8: return 4;
    case SDVL_BAYER_RGGB8: case SDVL_BAYER_GRBG8: case SDVL_BAYER_GBRG8: case SDVL_BAYER_BGGR8: return 1;
    case SDVL_YUYV8: case SDVL_UYVY8: case SDVL_GRAY10_16: case SDVL_GRAY12_16: case SDVL_GRAY16: return 2;
    default: return 0;
  }
}

bool is_bayer(int format) { return format >= SDVL_BAYER_RGGB8 && format <= SDVL_BAYER_BGGR8; }
bool is_yuv422(int format) { return format == SDVL_YUYV8 || format == SDVL_UYVY8; }
// depth - 8 of a 16-bit gray format, 0 for every other
int gray16_shift(int format) { return format == SDVL_GRAY10_16 ? 2 : format == SDVL_GRAY12_16 ? 4 : format == SDVL_GRAY16 ? 8 : 0; }

// what a format asks of an image's size beyond the entry's own limits; nullptr: nothing
const char *size_objection(int format, int w, int h) {
  if (is_bayer(format) && (w < 2 || h < 2)) return "a Bayer image size is at least 2 x 2";
  if (is_yuv422(format) && (w & 1)) return "YUYV / UYVY images have an even width";
  return nullptr;
}

template <int C>
__device__ __forceinline__ uint32_t byte_at(const uint32_t *dw, int k) { return (dw[k >> 2] >> (8 * (k & 3))) & 255u; }

// one workgroup = 256 lanes of one image (blockIdx.y); w0 / w2: the weights of bytes 0 and 2 of a pixel
template <int C>
__global__ __launch_bounds__(256) void to_gray_kernel(const GrayJob *__restrict__ jobs, int width, int height, int dstride, int w0, int w2) {
  const GrayJob job = jobs[blockIdx.y];
  if (job.mode != kScalar) {
    // (global address space: global_load / global_store with a scalar base instead of flat accesses)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4 *gsrc_t;
    typedef __attribute__((address_space(1))) u32x4 *gdst_t;
    const bool flat = job.mode == kFlat16;
    const int upr = flat ? static_cast<int>((static_cast<long long>(width) * height) >> 4) : width >> 4;  // 16-pixel units per row
    const long long units = flat ? upr : static_cast<long long>(upr) * height;
    for (long long u = blockIdx.x * 256 + threadIdx.x; u < units; u += 256LL * gridDim.x) {
      const int r = flat ? 0 : static_cast<int>(u / upr), c = static_cast<int>(u - static_cast<long long>(r) * upr);
      const gsrc_t s = (gsrc_t)(job.src + r * job.sstride + static_cast<long long>(c) * 16 * C);
      u32x4 a[C];
#pragma unroll
      for (int k = 0; k < C; k++) a[k] = __builtin_nontemporal_load(s + k);
      uint32_t dw[4 * C];
#pragma unroll
      for (int k = 0; k < C; k++) {
        dw[4 * k] = a[k].x; dw[4 * k + 1] = a[k].y; dw[4 * k + 2] = a[k].z; dw[4 * k + 3] = a[k].w;
      }
      uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
      for (int p = 0; p < 16; p++) {
        const uint32_t y = (byte_at<C>(dw, C * p) * w0 + byte_at<C>(dw, C * p + 1) * kW1 + byte_at<C>(dw, C * p + 2) * w2 + 8192u) >> 14;
        o[p >> 2] |= y << (8 * (p & 3));
      }
      u32x4 v;
      v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
      *(gdst_t)(job.dst + static_cast<long long>(r) * dstride + static_cast<long long>(c) * 16) = v;
    }
    return;
  }
  // odd strides, odd widths, unaligned sources: row by row, a pixel per lane
  for (int r = blockIdx.x; r < height; r += gridDim.x) {
    const uint8_t *s = job.src + r * job.sstride;
    uint8_t *d = job.dst + static_cast<long long>(r) * dstride;
    for (int x = threadIdx.x; x < width; x += 256) {
      const uint8_t *px = s + x * C;
      d[x] = static_cast<uint8_t>((px[0] * w0 + px[1] * kW1 + px[2] * w2 + 8192) >> 14);
    }
  }
}

// ---- two bytes per pixel: YUYV / UYVY (shift == 0: byte `ysel` of each pair is the gray) and little-endian 16-bit gray (shift = depth - 8:
// min(255, (v + half) >> shift)).  Launch-uniform arguments; the modes and the walk over an image are to_gray_kernel's.
template <bool U16>
__device__ __forceinline__ uint32_t narrow2(uint32_t lo, uint32_t hi, int ysel, int shift, uint32_t half) {
  if (U16) return min(255u, ((lo | (hi << 8)) + half) >> shift);
  return ysel ? hi : lo;
}

template <bool U16>
__global__ __launch_bounds__(256) void wide_gray_kernel(const GrayJob *__restrict__ jobs, int width, int height, int dstride, int ysel, int shift) {
  const GrayJob job = jobs[blockIdx.y];
  const uint32_t half = U16 ? 1u << (shift - 1) : 0u;
  if (job.mode != kScalar) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4 *gsrc_t;
    typedef __attribute__((address_space(1))) u32x4 *gdst_t;
    const bool flat = job.mode == kFlat16;
    const int upr = flat ? static_cast<int>((static_cast<long long>(width) * height) >> 4) : width >> 4;  // 16-pixel units per row
    const long long units = flat ? upr : static_cast<long long>(upr) * height;
    const int ybit = 8 * ysel;
    for (long long u = blockIdx.x * 256 + threadIdx.x; u < units; u += 256LL * gridDim.x) {
      const int r = flat ? 0 : static_cast<int>(u / upr), c = static_cast<int>(u - static_cast<long long>(r) * upr);
      const gsrc_t s = (gsrc_t)(job.src + r * job.sstride + static_cast<long long>(c) * 32);
      const u32x4 a0 = __builtin_nontemporal_load(s), a1 = __builtin_nontemporal_load(s + 1);
      const uint32_t dw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};  // a dword = two pixels
      uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
      for (int p = 0; p < 16; p++) {
        const uint32_t px = dw[p >> 1] >> (16 * (p & 1));
        const uint32_t y = U16 ? min(255u, ((px & 0xffffu) + half) >> shift) : (px >> ybit) & 255u;
        o[p >> 2] |= y << (8 * (p & 3));
      }
      u32x4 v;
      v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
      *(gdst_t)(job.dst + static_cast<long long>(r) * dstride + static_cast<long long>(c) * 16) = v;
    }
    return;
  }
  // odd strides, widths that are no multiple of 16, unaligned sources (a 16-bit image may even start at an odd address): byte accesses
  for (int r = blockIdx.x; r < height; r += gridDim.x) {
    const uint8_t *s = job.src + r * job.sstride;
    uint8_t *d = job.dst + static_cast<long long>(r) * dstride;
    for (int x = threadIdx.x; x < width; x += 256) d[x] = static_cast<uint8_t>(narrow2<U16>(s[2 * x], s[2 * x + 1], ysel, shift, half));
  }
}

// ---- Bayer mosaics.  k[2 (row & 1) + (column & 1)] = the weights of (m, Hh, Vv, D) at that position of the 2x2 tile
struct BayerCoef {
  int k[4][4];
};

// index i of a side of n >= 2 pixels, reflected without repeating the edge (i in -1 .. n + 1)
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

__device__ __forceinline__ uint32_t bayer_luma(const int *k, uint32_t m, uint32_t hh, uint32_t vv, uint32_t d) {
  return (m * k[0] + hh * k[1] + vv * k[2] + d * k[3] + 32768u) >> 16;
}

// byte j (-1 .. 16) of a 16-pixel row segment: its four dwords, the byte left of it and the byte right of it
__device__ __forceinline__ uint32_t seg_byte(const uint32_t *dw, uint32_t left, uint32_t right, int j) {
  return j < 0 ? left : j > 15 ? right : (dw[j >> 2] >> (8 * (j & 3))) & 255u;
}

__global__ __launch_bounds__(256) void bayer_gray_kernel(const GrayJob *__restrict__ jobs, int width, int height, int dstride, BayerCoef cf) {
  const GrayJob job = jobs[blockIdx.y];
  if (job.mode != kScalar) {  // kRows16: width, both strides and both addresses are multiples of 16
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4 *gsrc_t;
    typedef __attribute__((address_space(1))) u32x4 *gdst_t;
    const int upr = width >> 4, brows = (height + 1) >> 1;  // 16 x 2 blocks per row of blocks, rows of blocks
    const long long units = static_cast<long long>(upr) * brows;
    for (long long u = blockIdx.x * 256 + threadIdx.x; u < units; u += 256LL * gridDim.x) {
      const int br = static_cast<int>(u / upr), c = static_cast<int>(u - static_cast<long long>(br) * upr);
      const int r0 = 2 * br, x0 = 16 * c;
      // rows r0 - 1 .. r0 + 2 and the columns x0 - 1 and x0 + 16, reflected at the image's edges (all indices stay inside the image)
      const int rows[4] = {reflect(r0 - 1, height), r0, reflect(r0 + 1, height), reflect(r0 + 2, height)};
      const int xl = reflect(x0 - 1, width), xr = reflect(x0 + 16, width);
      uint32_t dw[4][4], left[4], right[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint8_t *row = job.src + rows[i] * job.sstride;
        const u32x4 a = *(gsrc_t)(row + x0);
        dw[i][0] = a.x; dw[i][1] = a.y; dw[i][2] = a.z; dw[i][3] = a.w;
        left[i] = row[xl];
        right[i] = row[xr];
      }
#pragma unroll
      for (int rr = 0; rr < 2; rr++) {  // output row r0 + rr: the segments above, at and below it are rr, rr + 1, rr + 2
        if (r0 + rr >= height) break;   // (the last row of blocks of an odd height)
        uint32_t vs[18];                // column sums above + below, columns -1 .. 16
#pragma unroll
        for (int j = -1; j <= 16; j++) vs[j + 1] = seg_byte(dw[rr], left[rr], right[rr], j) + seg_byte(dw[rr + 2], left[rr + 2], right[rr + 2], j);
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 16; p++) {
          const uint32_t m = seg_byte(dw[rr + 1], 0, 0, p);
          const uint32_t hh = seg_byte(dw[rr + 1], left[rr + 1], right[rr + 1], p - 1) + seg_byte(dw[rr + 1], left[rr + 1], right[rr + 1], p + 1);
          const uint32_t y = bayer_luma(cf.k[2 * rr + (p & 1)], m, hh, vs[p + 1], vs[p] + vs[p + 2]);
          o[p >> 2] |= y << (8 * (p & 3));
        }
        u32x4 v;
        v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
        *(gdst_t)(job.dst + static_cast<long long>(r0 + rr) * dstride + x0) = v;
      }
    }
    return;
  }
  // any width >= 2, stride and address: a pixel per lane, nine byte loads
  for (int r = blockIdx.x; r < height; r += gridDim.x) {
    const uint8_t *up = job.src + reflect(r - 1, height) * job.sstride, *mid = job.src + r * job.sstride;
    const uint8_t *down = job.src + reflect(r + 1, height) * job.sstride;
    uint8_t *d = job.dst + static_cast<long long>(r) * dstride;
    for (int x = threadIdx.x; x < width; x += 256) {
      const int xa = reflect(x - 1, width), xb = reflect(x + 1, width);
      const int cls = 2 * (r & 1) + (x & 1);
      const int k[4] = {cf.k[cls][0], cf.k[cls][1], cf.k[cls][2], cf.k[cls][3]};
      d[x] = static_cast<uint8_t>(bayer_luma(k, mid[x], static_cast<uint32_t>(mid[xa]) + mid[xb], static_cast<uint32_t>(up[x]) + down[x],
                                             static_cast<uint32_t>(up[xa]) + up[xb] + down[xa] + down[xb]));
    }
  }
}

// the table of a Bayer order: red at (rr, rc) of the tile, blue diagonally opposite.  An R or B site: its own colour from m, green from
// Hh + Vv, the opposite colour from D.  A G site: green from 4 m, the row's other colour from 2 Hh, the column's from 2 Vv.
BayerCoef bayer_coef(int format) {
  const int rr = (format == SDVL_BAYER_GBRG8 || format == SDVL_BAYER_BGGR8) ? 1 : 0;
  const int rc = (format == SDVL_BAYER_GRBG8 || format == SDVL_BAYER_BGGR8) ? 1 : 0;
  BayerCoef cf;
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 2; c++) {
      int *k = cf.k[2 * r + c];
      const bool red = r == rr && c == rc, blue = r != rr && c != rc;
      if (red || blue) {
        k[0] = 4 * (red ? kWR : kWB); k[1] = kW1; k[2] = kW1; k[3] = red ? kWB : kWR;
      } else {
        const bool red_row = r == rr;
        k[0] = 4 * kW1; k[1] = 2 * (red_row ? kWR : kWB); k[2] = 2 * (red_row ? kWB : kWR); k[3] = 0;
      }
    }
  return cf;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// n colour images -> n gray images (device, row stride dst_stride), on ctx->stream.  dst == nullptr: the gray images go to the front of
// the context's scratch (row stride w, 256-byte aligned) and `scratch_dst` receives where; staged copies of pageable sources (and of every
// Bayer source in host memory: its rows are read three times) follow them.
int run_to_gray(sdvl_ctx *ctx, int n, const void *const *src, int src_stride, int src_on_device, int w, int h, int format,
                uint8_t *const *dst, int dst_stride, std::vector<uint8_t *> *scratch_dst) {
  const int C = channels_of(format);
  const size_t row_bytes = static_cast<size_t>(w) * C, img_bytes = row_bytes * h;
  SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
  std::vector<const uint8_t *> srcs(n);
  std::vector<long long> strides(n, src_stride);
  std::vector<int> staged;
  const bool bayer = is_bayer(format);
  for (int i = 0; i < n; i++) {
    if (src_on_device) {
      srcs[i] = static_cast<const uint8_t *>(src[i]);
      continue;
    }
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, src[i]) == hipSuccess && ((attr.type == hipMemoryTypeHost && !bayer) || attr.type == hipMemoryTypeDevice) &&
        attr.devicePointer) {  // pinned host memory (or HBM): read in place over the link
      srcs[i] = static_cast<const uint8_t *>(attr.devicePointer);
    } else {
      (void)hipGetLastError();  // an unregistered pointer is not an error here
      staged.push_back(i);
    }
  }
  const size_t gray_pitch = sdvl_align256(static_cast<size_t>(w) * h), pitch = sdvl_align256(img_bytes);
  sdvl_layout wk;  // d_work: the gray images (when the caller gave no destinations) | tight copies of the pageable sources
  const sdvl_part<uint8_t> wk_gray = wk.take<uint8_t>(dst ? 0 : gray_pitch * n), wk_staged = wk.take<uint8_t>(pitch * staged.size());
  if (wk.bytes() > 0) {
    int rc = sdvl_ensure(ctx, &ctx->d_work, &ctx->d_work_bytes, wk.bytes(), false);
    if (rc) return rc;
  }
  if (!dst) {
    scratch_dst->resize(n);
    for (int i = 0; i < n; i++) (*scratch_dst)[i] = wk_gray.in(ctx->d_work) + gray_pitch * i;
    dst = scratch_dst->data();
    dst_stride = w;
  }
  if (!staged.empty()) {  // pageable (Bayer: any host memory): a tight copy in the context's scratch first
    // tight images that follow each other in host memory (a camera's buffer pool, a batch read in one piece) go as ONE copy: a copy per
    // 300 KB image costs more in its call than in its bytes
    const bool joinable = static_cast<size_t>(src_stride) == row_bytes && pitch == img_bytes;
    for (size_t k = 0; k < staged.size();) {
      size_t run = 1;
      while (joinable && k + run < staged.size() &&
             static_cast<const uint8_t *>(src[staged[k + run]]) == static_cast<const uint8_t *>(src[staged[k + run - 1]]) + img_bytes)
        run++;
      uint8_t *d = wk_staged.in(ctx->d_work) + pitch * k;
      if (joinable) SDVL_HIP_CHECK(ctx, hipMemcpyAsync(d, src[staged[k]], img_bytes * run, hipMemcpyHostToDevice, ctx->stream));
      else SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(d, row_bytes, src[staged[k]], src_stride, row_bytes, h, hipMemcpyHostToDevice, ctx->stream));
      for (size_t j = 0; j < run; j++) {
        srcs[staged[k + j]] = d + pitch * j;
        strides[staged[k + j]] = static_cast<long long>(row_bytes);
      }
      k += run;
    }
  }
  const size_t jb = sizeof(GrayJob) * n;
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_stage_alloc(ctx, jb, &hs, &dsx);
  if (rc) return rc;
  GrayJob *hj = static_cast<GrayJob *>(hs);
  const bool dense_px = ((static_cast<size_t>(w) * h) & 15u) == 0;
  for (int i = 0; i < n; i++) {
    int mode = kScalar;
    if (aligned16(srcs[i]) && aligned16(dst[i])) {
      if (strides[i] == static_cast<long long>(row_bytes) && dst_stride == w && dense_px && !bayer) mode = kFlat16;  // (Bayer: 2-D blocks)
      else if ((w & 15) == 0 && (strides[i] & 15) == 0 && (dst_stride & 15) == 0) mode = kRows16;
    }
    hj[i] = GrayJob{srcs[i], dst[i], strides[i], mode, 0};
  }
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, jb));
  const bool bgr = format == SDVL_BGR8 || format == SDVL_BGRA8;
  const int w0 = bgr ? kWB : kWR, w2 = bgr ? kWR : kWB;
  const long long units = bayer ? static_cast<long long>((w + 15) >> 4) * ((h + 1) >> 1) : (static_cast<long long>(w) * h) >> 4;
  const int shift = gray16_shift(format), ysel = format == SDVL_UYVY8 ? 1 : 0;
  const BayerCoef cf = bayer_coef(format);
  const int gx = static_cast<int>(std::max(1LL, std::min<long long>((units + 255) / 256, kMaxChunks)));
  constexpr int kMaxJobsPerLaunch = 32768;  // (grid y)
  for (int i0 = 0; i0 < n; i0 += kMaxJobsPerLaunch) {
    const int m = std::min(kMaxJobsPerLaunch, n - i0);
    const GrayJob *jobs = static_cast<const GrayJob *>(dsx) + i0;
    if (bayer) SDVL_LAUNCH(ctx, "bayer_gray", bayer_gray_kernel, dim3(gx, m), dim3(256), jobs, w, h, dst_stride, cf);
    else if (shift) SDVL_LAUNCH(ctx, "wide_gray", wide_gray_kernel<true>, dim3(gx, m), dim3(256), jobs, w, h, dst_stride, 0, shift);
    else if (C == 2) SDVL_LAUNCH(ctx, "wide_gray", wide_gray_kernel<false>, dim3(gx, m), dim3(256), jobs, w, h, dst_stride, ysel, 0);
    else if (C == 3) SDVL_LAUNCH(ctx, "to_gray", to_gray_kernel<3>, dim3(gx, m), dim3(256), jobs, w, h, dst_stride, w0, w2);
    else SDVL_LAUNCH(ctx, "to_gray", to_gray_kernel<4>, dim3(gx, m), dim3(256), jobs, w, h, dst_stride, w0, w2);
  }
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  return SDVL_OK;
}

// the frame records of an upload (what sdvl_frames_upload does to a frame besides the pixels)
void frame_takes_new_image(sdvl_frame *f) {
  f->v.level[0] = f->own_level0;
  f->hdr_stale = 1;
  f->v.n_corners = 0;
  f->desc_valid = 0;
  f->bins_valid = 0;
}

}  // namespace

extern "C" {

int sdvl_convert_gray(sdvl_ctx *ctx, int n, const void *const *src, int src_stride, int src_on_device, int width, int height, int format,
                      void *const *dst_dev, int dst_stride) {
  if (!ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, n >= 0 && (n == 0 || (src && dst_dev)), "sdvl_convert_gray: null image list");
  const int C = channels_of(format);
  SDVL_REQUIRE(ctx, C > 0, "sdvl_convert_gray: unknown pixel format");
  SDVL_REQUIRE(ctx, width >= 1 && height >= 1 && width <= kMaxSide && height <= kMaxSide, "sdvl_convert_gray: image size out of range (1 .. 16384 a side)");
  SDVL_REQUIRE(ctx, !size_objection(format, width, height), std::string("sdvl_convert_gray: ") + size_objection(format, width, height));
  SDVL_REQUIRE(ctx, static_cast<long long>(src_stride) >= static_cast<long long>(width) * C, "sdvl_convert_gray: source stride smaller than width x bytes per pixel");
  SDVL_REQUIRE(ctx, dst_stride >= width, "sdvl_convert_gray: destination stride smaller than width");
  for (int i = 0; i < n; i++) SDVL_REQUIRE(ctx, src[i] && dst_dev[i] && src[i] != dst_dev[i], "sdvl_convert_gray: null image or in-place conversion");
  if (n == 0) return SDVL_OK;
  if (format == SDVL_GRAY8) {  // the gray entries' copy (sdvl_undistort without a lens)
    SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
    for (int i = 0; i < n; i++)
      SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(dst_dev[i], dst_stride, src[i], src_stride, width, height,
                                           src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return SDVL_OK;
  }
  return run_to_gray(ctx, n, src, src_stride, src_on_device, width, height, format, reinterpret_cast<uint8_t *const *>(dst_dev), dst_stride, nullptr);
}

// `rect` (a rectified camera, sdvl_frames_upload_color_rectified) takes the place of the lens: where the upload routes to the
// undistorted upload it routes to the rectified one
static int upload_color(sdvl_ctx *ctx, int n, sdvl_frame *const *frames, const void *const *src, int src_stride, int src_on_device,
                        int format, const sdvl_camera *cam, const sdvl_distortion *dist, const sdvl_rectification *rect) {
  if (!ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, n >= 0 && (n == 0 || (frames && src)), "sdvl_frames_upload_color: null frame or image list");
  const int C = channels_of(format);
  SDVL_REQUIRE(ctx, C > 0, "sdvl_frames_upload_color: unknown pixel format");
  SDVL_REQUIRE(ctx, (cam == nullptr) == (dist == nullptr), "sdvl_frames_upload_color: pass both cam and dist, or neither");
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, frames[0] != nullptr, "sdvl_frames_upload_color: null frame or image");
  const int w = frames[0]->width, h = frames[0]->height;
  for (int i = 0; i < n; i++) {
    SDVL_REQUIRE(ctx, frames[i] && src[i], "sdvl_frames_upload_color: null frame or image");
    SDVL_REQUIRE(ctx, frames[i]->width == w && frames[i]->height == h, "sdvl_frames_upload_color: frames of one call share a size");
    SDVL_REQUIRE(ctx, src[i] != frames[i]->own_level0, "sdvl_frames_upload_color: in-place conversion");
  }
  SDVL_REQUIRE(ctx, !size_objection(format, w, h), std::string("sdvl_frames_upload_color: ") + size_objection(format, w, h));
  SDVL_REQUIRE(ctx, static_cast<long long>(src_stride) >= static_cast<long long>(w) * C, "sdvl_frames_upload_color: source stride smaller than width x bytes per pixel");
  const bool lens = rect || (dist && dist->d[0] != 0.0);  // Camera::SetDistortions tests d0 only (camera.cc:46)
  const auto remapped_upload = [&](const void *const *gray, int gray_stride, int gray_on_device) {
    if (rect) return sdvl_frames_upload_rectified(ctx, n, frames, gray, gray_stride, gray_on_device, rect);
    return sdvl_frames_upload_undistorted(ctx, n, frames, gray, gray_stride, gray_on_device, cam, dist);
  };
  if (format == SDVL_GRAY8) {  // exactly the gray producers
    if (lens) return remapped_upload(src, src_stride, src_on_device);
    return sdvl_frames_upload(ctx, n, frames, reinterpret_cast<const uint8_t *const *>(src), src_stride);
  }
  SDVL_REQUIRE(ctx, w <= kMaxSide && h <= kMaxSide, "sdvl_frames_upload_color: image size out of range");
  if (!lens) {  // gray straight into the frames' level 0
    std::vector<uint8_t *> dst(n);
    for (int i = 0; i < n; i++) dst[i] = frames[i]->own_level0;
    const int rc = run_to_gray(ctx, n, src, src_stride, src_on_device, w, h, format, dst.data(), w, nullptr);
    if (rc) return rc;
    for (int i = 0; i < n; i++) frame_takes_new_image(frames[i]);
    return SDVL_OK;
  }
  // with a lens: gray into the scratch the remap reads raw sources from, then the unchanged remap writes level 0
  std::vector<uint8_t *> gray;
  const int rc = run_to_gray(ctx, n, src, src_stride, src_on_device, w, h, format, nullptr, w, &gray);
  if (rc) return rc;
  std::vector<const void *> gsrc(gray.begin(), gray.end());
  return remapped_upload(gsrc.data(), w, 1);
}

int sdvl_frames_upload_color(sdvl_ctx *ctx, int n, sdvl_frame *const *frames, const void *const *src, int src_stride, int src_on_device,
                             int format, const sdvl_camera *cam, const sdvl_distortion *dist) {
  return upload_color(ctx, n, frames, src, src_stride, src_on_device, format, cam, dist, nullptr);
}

int sdvl_frames_upload_color_rectified(sdvl_ctx *ctx, int n, sdvl_frame *const *frames, const void *const *src, int src_stride,
                                       int src_on_device, int format, const sdvl_rectification *r) {
  if (!ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, r != nullptr, "sdvl_frames_upload_color_rectified: null rectification");
  return upload_color(ctx, n, frames, src, src_stride, src_on_device, format, nullptr, nullptr, r);
}

}  // extern "C"
