// sdvl_undistort.hip — K0 input stage: Camera::UndistortImage = cv::undistort(in, out, K, D) (camera.cc:39-67,100-105,
// main.cc:133) as a remap from a CACHED per-camera map, optionally fused with the upload into a frame's level 0.
//
// cv::undistort builds, stripe by stripe, a fixed-point map with cv::initUndistortRectifyMap and feeds it to cv::remap
// (bilinear, BORDER_CONSTANT 0).  Nothing in that map depends on the image — Camera::SetDistortions fixes it for the life of the
// camera (camera.cc:39-67) — so it is built ONCE per (camera, distortion, size) and context, on the device, in exactly the library's
// arithmetic: the host prepares
//   xw[j] = normalised x of column j   (the library accumulates _x += ir[0] along the row: sequential rounding),
//   yw[r] = normalised y of row r      (with the principal point of the row's STRIPE, Ar(1,2) = v0 - y0),
// undistort_map_kernel evaluates the radial-tangential model per pixel in FP64 (-ffp-contract=off, the library's expression order),
// iu = cvRound(32 u), and packs integer part + 5-bit fractions into one 32-bit word per pixel (1.2 MB for 640x480: it stays in L2
// across the frames of a launch).  undistort_remap_kernel is then an integer gather: a lane takes four adjacent output pixels of
// four frames — map words decoded once, 15-bit weight table entry, 4 taps, (sum + 2^14) >> 15, one 32-bit store per frame.
// HBM-bound: one u8 neighbourhood read and one u8 write per pixel (2 W H algorithmic bytes per frame).
// Round 5's kernel recomputed the FP64 model for every pixel of every frame: 282 us per 256 frames of 640x480 (0.07 of HBM).
//
// Stereo rigs as calibrated (sdvl_rectify, sdvl_frames_upload_rectified): rectification is the same remap behind another map — where
// cv::undistort passes the identity and K, a rectified camera has a rotation R_i and new intrinsics.  rectify_map_kernel writes that map
// in the same words, undistort_quad_kernel and undistort_remap_kernel consume it unchanged, one launch per camera.  Those maps are kept in a
// cache of their own (sdvl_ctx::rect_maps); the undistortion's single slot and its counter stay as they were.
#include <cmath>
#include <cstring>
#include <vector>

#include "sdvl_internal.h"

namespace {

struct UndistJob {
  const uint8_t *src;
  uint8_t *dst;
};

struct UndistParams {
  double fx, fy, u0, v0, k1, k2, p1, p2, k3;
  int w, h, sstride, dstride;
};

constexpr int kMapMax = 2044;      // the packed map: integer parts are stored with 11 bits each (clamped to [-2, size], + 2)
constexpr int kMapMaxWide = 4095;  // the wide map (frames with a side above 2044, up to the frames' own limit): 16 bits each

// map word: a | b << 5 | (clamp(sx, -2, W) + 2) << 10 | (clamp(sy, -2, H) + 2) << 21.  sx <= -2 or sx >= W (likewise sy) puts all four
// taps outside the image, so the clamp loses nothing.  Row pitch = W rounded up to 4 pixels; the padding says "outside".
// The wide map (kWideMap) keeps two words per pixel: a | b << 5, then (clamp(sx, -2, W) + 2) | (clamp(sy, -2, H) + 2) << 16.
template <bool kWideMap>
__device__ __forceinline__ void map_store(uint32_t *map, size_t px, uint32_t a, uint32_t b, uint32_t sxc, uint32_t syc) {
  if (kWideMap)
    *reinterpret_cast<uint2 *>(map + 2 * px) = make_uint2(a | b << 5, sxc | syc << 16);
  else
    map[px] = a | b << 5 | sxc << 10 | syc << 21;
}

// the entries of four adjacent pixels (px a multiple of 4): fractions and source positions (sx, sy), -2 .. size
template <bool kWideMap>
__device__ __forceinline__ void map_load4(const uint32_t *map, size_t px, uint32_t a[4], uint32_t b[4], int sx[4], int sy[4]) {
  if (kWideMap) {
    const uint4 w01 = *reinterpret_cast<const uint4 *>(map + 2 * px), w23 = *reinterpret_cast<const uint4 *>(map + 2 * px + 4);
    const uint32_t lo[4] = {w01.x, w01.z, w23.x, w23.z}, hi[4] = {w01.y, w01.w, w23.y, w23.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      a[k] = lo[k] & 31u;
      b[k] = (lo[k] >> 5) & 31u;
      sx[k] = static_cast<int>(hi[k] & 0xFFFFu) - 2;
      sy[k] = static_cast<int>(hi[k] >> 16) - 2;
    }
  } else {
    const uint4 words = *reinterpret_cast<const uint4 *>(map + px);
    const uint32_t wd[4] = {words.x, words.y, words.z, words.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      a[k] = wd[k] & 31u;
      b[k] = (wd[k] >> 5) & 31u;
      sx[k] = static_cast<int>((wd[k] >> 10) & 2047u) - 2;
      sy[k] = static_cast<int>(wd[k] >> 21) - 2;
    }
  }
}

// the map entry of the ray (x, y, 1): the radial-tangential model in the library's expression order, fixed-point position, the word's
// parts.  Returns whether one of the entry's four taps lies outside the image
__device__ __forceinline__ bool map_entry(const UndistParams &P, double x, double y, uint32_t *fa, uint32_t *fb, uint32_t *sxc, uint32_t *syc) {
  const double x2 = x * x, y2 = y * y;
  const double r2 = x2 + y2, _2xy = 2 * x * y;
  const double k4 = 0, k5 = 0, k6 = 0;
  const double kr = (1 + ((P.k3 * r2 + P.k2) * r2 + P.k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
  const double u = P.fx * (x * kr + P.p1 * _2xy + P.p2 * (r2 + 2 * x2)) + P.u0;
  const double v = P.fy * (y * kr + P.p1 * (r2 + 2 * y2) + P.p2 * _2xy) + P.v0;
  const int iu = __double2int_rn(u * 32), iv = __double2int_rn(v * 32);  // cvRound = round half to even
  const int sx = static_cast<short>(iu >> 5), sy = static_cast<short>(iv >> 5);
  *fa = static_cast<uint32_t>(iu & 31);
  *fb = static_cast<uint32_t>(iv & 31);
  *sxc = static_cast<uint32_t>(min(max(sx, -2), P.w) + 2);
  *syc = static_cast<uint32_t>(min(max(sy, -2), P.h) + 2);
  return sx < 0 || sy < 0 || sx + 1 >= P.w || sy + 1 >= P.h;
}

template <bool kWideMap>
__global__ __launch_bounds__(256) void undistort_map_kernel(const double *__restrict__ xw, const double *__restrict__ yw, UndistParams P, int pitch,
                                                            uint32_t *__restrict__ map) {
  const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (j >= pitch) return;
  uint32_t fa = 0, fb = 0, sxc = 0, syc = 0;  // sx = sy = -2: outside
  if (j < P.w) map_entry(P, xw[j], yw[r], &fa, &fb, &sxc, &syc);
  map_store<kWideMap>(map, static_cast<size_t>(r) * pitch + j, fa, fb, sxc, syc);
}

// The map of a RECTIFIED camera, the sibling of undistort_map_kernel: the ray of output pixel (j, r) is M (j, r, 1) with M = R_i^T
// K_rect^-1 (host, FP64), evaluated directly — M is full, so the library's accumulation along a row (xw / yw above) has no per-row and
// per-column table to live in — then the same entry.  A ray that does not point forward in the raw camera's frame (w <= 0, or not a
// number: a large turn, a wide override) has no source: the entry says "outside", it is not left to what x / w converts to.  The kernel
// also counts the pixels with a tap outside the raw image: one ballot and one atomic add per wave.
struct RectifyRays {
  double M[9];
};

template <bool kWideMap>
__global__ __launch_bounds__(256) void rectify_map_kernel(RectifyRays rays, UndistParams P, int pitch, uint32_t *__restrict__ map,
                                                          unsigned int *__restrict__ no_source) {
  const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  uint32_t fa = 0, fb = 0, sxc = 0, syc = 0;  // sx = sy = -2: outside
  bool outside = false;
  if (j < P.w) {
    const double *M = rays.M;
    const double x = M[0] * j + M[1] * r + M[2], y = M[3] * j + M[4] * r + M[5], w = M[6] * j + M[7] * r + M[8];
    outside = !(w > 0) || map_entry(P, x / w, y / w, &fa, &fb, &sxc, &syc);  // (w <= 0: the entry stays "outside")
  }
  if (j < pitch) map_store<kWideMap>(map, static_cast<size_t>(r) * pitch + j, fa, fb, sxc, syc);
  const unsigned long long votes = __ballot(outside);  // (every lane of the wave arrives here)
  if (votes != 0 && (threadIdx.x & 63) == 0) atomicAdd(no_source, static_cast<unsigned int>(__popcll(votes)));
}

// The remap proper works on QUADS of adjacent output pixels.  The map moves by about a pixel per pixel, so the source pixels of a quad
// lie within 8 bytes of at most THREE consecutive rows (rows y0, y0 + 1 for most quads; where the map crosses a source row inside the
// quad, some of its pixels start at y0 + 1).  undistort_quad_kernel notes that once per camera in a 16-byte record:
//   off   where the quad's 8-byte window starts in the source image (first row; both clamped into the image)
//   sel   3-bit byte selectors of the left and of the right tap of each pixel inside the window, the pixels' row bits (sy_k - y0),
//         and whether the second / third row lie one stride further (they do not where the window is clamped at the image's edge)
//   a, b  the 5-bit fractions of the four pixels, and one VALID bit per tap
// cv::remap's BORDER_CONSTANT 0 reads a tap outside the image as 0: here such a tap has weight 0 and selects some byte of the
// (clamped) window.  The remap of a quad of a frame is then three unaligned 8-byte loads (the amdhsa ABI runs with unaligned access
// on), six byte permutes, four bit selects and 16 multiply-adds — no branch, border or not.
// BilinearTab_i[b * 32 + a] is 32 x {(32-b)(32-a), (32-b)a, b(32-a), ba}, so (sum + 2^14) >> 15 equals
// (S0 (32-b)(32-a) + S1 (32-b) a + S2 b (32-a) + S3 b a + 512) >> 10 — also for the table's repaired (0,0) entry {32767, 0, 0, 1}
// (saturate_cast<short>(32768) and the sum repair as OpenCV builds it): with S3 - S0 + 16384 in [16129, 16639] it yields S0, like weight
// 1024 on S0 alone, and 0 when S0 lies outside.  A quad whose live taps do not fit the window (a map that jumps: no camera's) takes the
// tap-by-tap path from the per-pixel words.
struct QuadRec {
  int off;
  uint32_t sel;  // [0:12) selL x 4, [12:24) selR x 4, [24:28) row bits, 28: row b = row a + stride, 29: row c = row b + stride; ~0: not compact
  uint32_t a;    // [0:20) a x 4, [20:32) valid bits of pixels 0..2 (bit 4k + i: tap i of pixel k; taps: 0 top left, 1 top right, 2 bottom left, 3 bottom right)
  uint32_t b;    // [0:20) b x 4, [20:24) valid bits of pixel 3
};

template <bool kWideMap>
__global__ __launch_bounds__(256) void undistort_quad_kernel(const uint32_t *__restrict__ map, int pitch, UndistParams P, QuadRec *__restrict__ quads) {
  const int qx = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, nq = pitch / 4;
  if (qx >= nq) return;
  const int W = P.w, H = P.h, ss = P.sstride;
  int sx[4], sy[4];
  uint32_t fa[4], fb[4];
  map_load4<kWideMap>(map, static_cast<size_t>(r) * pitch + 4 * qx, fa, fb, sx, sy);
  uint32_t valid = 0, qa = 0, qb = 0;
  int xlo = 1 << 20, xhi = -(1 << 20), y0 = 1 << 20, y1 = -(1 << 20);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    qa |= fa[k] << (5 * k);
    qb |= fb[k] << (5 * k);
    bool live = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int x = sx[k] + (i & 1), y = sy[k] + (i >> 1);
      if (x >= 0 && y >= 0 && x < W && y < H) {
        valid |= 1u << (4 * k + i);
        xlo = min(xlo, x);
        xhi = max(xhi, x);
        live = true;
      }
    }
    if (live) {
      y0 = min(y0, sy[k]);
      y1 = max(y1, sy[k]);
    }
  }
  QuadRec q;
  q.a = qa | (valid & 0xFFFu) << 20;
  q.b = qb | (valid >> 12) << 20;
  if (valid == 0) {  // nothing of the quad lies inside the image: all weights 0, any window
    q.off = 0;
    q.sel = 0;
  } else {
    const int xwin = min(xlo, W - 8);
    if (W < 8 || y1 - y0 > 1 || xhi - xwin > 7) {
      q.off = 0;
      q.sel = ~0u;
    } else {
      const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1), yc = min(max(y0 + 2, 0), H - 1);
      uint32_t sel = (yb != ya ? 1u << 28 : 0u) | (yc != yb ? 1u << 29 : 0u);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool live = ((valid >> (4 * k)) & 15u) != 0;
        sel |= static_cast<uint32_t>(min(max(sx[k] - xwin, 0), 7)) << (3 * k);
        sel |= static_cast<uint32_t>(min(max(sx[k] + 1 - xwin, 0), 7)) << (12 + 3 * k);
        if (live && sy[k] != y0) sel |= 1u << (24 + k);
      }
      q.off = ya * ss + xwin;
      q.sel = sel;
    }
  }
  quads[static_cast<size_t>(r) * nq + qx] = q;
}

// (S0 p0 + S1 p1 + S2 p2 + S3 p3 + 512) >> 10 for pixel k of a quad: Lt / Rt = left / right taps of its upper row as packed bytes, Lb / Rb of the lower
// (every product is below 2^18: the 24-bit multiplier with byte selects, not the quarter-rate 32-bit one)
template <int k>
__device__ __forceinline__ uint32_t quad_px(uint32_t Lt, uint32_t Rt, uint32_t Lb, uint32_t Rb, const uint32_t *p) {
  return (__umul24((Lt >> (8 * k)) & 255u, p[0]) + __umul24((Rt >> (8 * k)) & 255u, p[1]) + __umul24((Lb >> (8 * k)) & 255u, p[2]) +
          __umul24((Rb >> (8 * k)) & 255u, p[3]) + 512u) >> 10;
}

__device__ __forceinline__ uint32_t bit_select(uint32_t mask, uint32_t one, uint32_t zero) { return (mask & one) | (~mask & zero); }  // v_bfi_b32
__device__ __forceinline__ uint32_t spread3(uint32_t f) {  // four 3-bit fields -> the low bits of four bytes
  return (f & 7u) | ((f >> 3) & 7u) << 8 | ((f >> 6) & 7u) << 16 | ((f >> 9) & 7u) << 24;
}

// one workgroup = a tile of 128 x 8 output pixels (a lane: one quad) of kRemapFrames consecutive frames; the loads of all frames of the
// lane are in flight before the first result is needed.  kFull: all kRemapFrames frames exist (every workgroup but the last frame group's);
// kWide: every destination row start is 4-byte aligned and a multiple of four pixels wide (the frames' own level 0 always is)
constexpr int kRemapFrames = 4;
template <bool kFull, bool kWide>
__device__ __forceinline__ void remap_compact(const UndistJob *__restrict__ jobs, const QuadRec q, int nf, int ss, uint32_t drow, int npx) {
  // (the frame pointers are uniform and name global memory: address space 1 lets the loads take a scalar base + 32-bit lane offset
  //  instead of a 64-bit flat address per lane)
  typedef const __attribute__((address_space(1))) uint8_t *gsrc_t;
  typedef __attribute__((address_space(1))) uint8_t *gdst_t;
  typedef unsigned long long __attribute__((aligned(1))) u64_any;  // (an 8-byte window at any byte address)
  typedef const __attribute__((address_space(1))) u64_any *gwin_t;
  unsigned long long ra[kRemapFrames], rb[kRemapFrames], rc[kRemapFrames];
  gdst_t dst[kRemapFrames];
  const uint32_t off_a = static_cast<uint32_t>(q.off), off_b = off_a + ((q.sel >> 28) & 1u ? ss : 0), off_c = off_b + ((q.sel >> 29) & 1u ? ss : 0);
#pragma unroll
  for (int k = 0; k < kRemapFrames; k++) {
    const UndistJob job = jobs[kFull ? k : min(k, nf - 1)];
    const gsrc_t src = (gsrc_t)job.src;
    ra[k] = *(gwin_t)(src + off_a);
    rb[k] = *(gwin_t)(src + off_b);
    rc[k] = *(gwin_t)(src + off_c);
    dst[k] = (gdst_t)job.dst;
  }
  // the sixteen weights of the quad: p0 = (32-b)(32-a), p1 = (32-b) a, p2 = b (32-a), p3 = b a; 0 for a tap outside the image
  uint32_t p[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t a = (q.a >> (5 * k)) & 31u, b = (q.b >> (5 * k)) & 31u;
    p[k][0] = (32u - b) * (32u - a);
    p[k][1] = (32u - b) * a;
    p[k][2] = b * (32u - a);
    p[k][3] = b * a;
  }
  const uint32_t valid = (q.a >> 20) | ((q.b >> 20) & 15u) << 12;
  if (valid != 0xFFFFu) {
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (!((valid >> (4 * k + i)) & 1u)) p[k][i] = 0;
  }
  const uint32_t selL = spread3(q.sel), selR = spread3(q.sel >> 12);
  const uint32_t rowbits = (q.sel >> 24) & 15u;
  const uint32_t rowbyte = (rowbits | rowbits << 7 | rowbits << 14 | rowbits << 21) & 0x01010101u;
  const uint32_t M = (rowbyte << 8) - rowbyte;  // 0xFF in the bytes of the pixels that start one row lower
#pragma unroll
  for (int k = 0; k < kRemapFrames; k++) {
    if (!kFull && k >= nf) break;
    const uint32_t alo = static_cast<uint32_t>(ra[k]), ahi = static_cast<uint32_t>(ra[k] >> 32);
    const uint32_t blo = static_cast<uint32_t>(rb[k]), bhi = static_cast<uint32_t>(rb[k] >> 32);
    const uint32_t clo = static_cast<uint32_t>(rc[k]), chi = static_cast<uint32_t>(rc[k] >> 32);
    const uint32_t La = __builtin_amdgcn_perm(ahi, alo, selL), Ra = __builtin_amdgcn_perm(ahi, alo, selR);
    const uint32_t Lb = __builtin_amdgcn_perm(bhi, blo, selL), Rb = __builtin_amdgcn_perm(bhi, blo, selR);
    const uint32_t Lc = __builtin_amdgcn_perm(chi, clo, selL), Rc = __builtin_amdgcn_perm(chi, clo, selR);
    const uint32_t Lt = bit_select(M, Lb, La), Rt = bit_select(M, Rb, Ra), Lu = bit_select(M, Lc, Lb), Ru = bit_select(M, Rc, Rb);
    const uint32_t q0 = quad_px<0>(Lt, Rt, Lu, Ru, p[0]), q1 = quad_px<1>(Lt, Rt, Lu, Ru, p[1]);
    const uint32_t q2 = quad_px<2>(Lt, Rt, Lu, Ru, p[2]), q3 = quad_px<3>(Lt, Rt, Lu, Ru, p[3]);
    gdst_t d = dst[k] + drow;
    if (kWide) {
      *(__attribute__((address_space(1))) uint32_t *)d = q0 | q1 << 8 | q2 << 16 | q3 << 24;
    } else {
      d[0] = static_cast<uint8_t>(q0);
      if (npx > 1) d[1] = static_cast<uint8_t>(q1);
      if (npx > 2) d[2] = static_cast<uint8_t>(q2);
      if (npx > 3) d[3] = static_cast<uint8_t>(q3);
    }
  }
}

template <bool kWideMap>
__global__ __launch_bounds__(256) void undistort_remap_kernel(const UndistJob *__restrict__ jobs, const uint32_t *__restrict__ map,
                                                              const QuadRec *__restrict__ quads, int pitch, int n, int wide, UndistParams P) {
  // Workgroups are dealt to the eight XCDs round robin by their linear id: the frame group is the FASTEST index, so an XCD (its L2)
  // sees all tiles of one eighth of the frames and neighbouring tiles of a frame — which share source lines — meet in one L2.
  // (grid = frame groups x tiles across x tiles down: x is the fastest index of the dispatch order)
  const int zi = blockIdx.x;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int j0 = (blockIdx.y * 32 + tx) * 4, r = blockIdx.z * 8 + ty;
  if (j0 >= P.w || r >= P.h) return;
  const int W = P.w, H = P.h, ss = P.sstride;
  const int f0 = zi * kRemapFrames, nf = min(n - f0, kRemapFrames);
  const uint32_t drow = static_cast<uint32_t>(r) * P.dstride + j0;  // (images of at most 4095 x 4095: 32 bits)
  const QuadRec q = quads[static_cast<size_t>(r) * (pitch / 4) + (j0 >> 2)];
  const int npx = min(4, W - j0);
  if (q.sel != ~0u) {
    if (nf == kRemapFrames) {
      if (wide) remap_compact<true, true>(jobs + f0, q, nf, ss, drow, npx);
      else remap_compact<true, false>(jobs + f0, q, nf, ss, drow, npx);
    } else {
      remap_compact<false, false>(jobs + f0, q, nf, ss, drow, npx);
    }
    return;
  }
  // A quad whose live taps do not fit one window: tap by tap from the per-pixel words, the same way — a tap outside the image has
  // weight 0 and an address clamped into the image, decided once per lane.
  uint32_t fa[4], fb[4];
  int psx[4], psy[4];
  map_load4<kWideMap>(map, static_cast<size_t>(r) * pitch + j0, fa, fb, psx, psy);
  uint32_t off[4][4], wt[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t a = fa[k], b = fb[k];
    const int sx = psx[k], sy = psy[k];
    const uint32_t pw[4] = {(32u - b) * (32u - a), (32u - b) * a, b * (32u - a), b * a};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int x = sx + (i & 1), y = sy + (i >> 1);
      const bool inside = x >= 0 && y >= 0 && x < W && y < H;
      off[k][i] = static_cast<uint32_t>(min(max(y, 0), H - 1)) * ss + min(max(x, 0), W - 1);
      wt[k][i] = inside ? pw[i] : 0u;
    }
  }
  typedef const __attribute__((address_space(1))) uint8_t *gsrc_t;
  typedef __attribute__((address_space(1))) uint8_t *gdst_t;
  for (int f = 0; f < nf; f++) {
    const UndistJob job = jobs[f0 + f];
    const gsrc_t src = (gsrc_t)job.src;
    uint32_t qv[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      qv[k] = (__umul24(src[off[k][0]], wt[k][0]) + __umul24(src[off[k][1]], wt[k][1]) + __umul24(src[off[k][2]], wt[k][2]) + __umul24(src[off[k][3]], wt[k][3]) + 512u) >> 10;
    gdst_t d = (gdst_t)job.dst + drow;
    d[0] = static_cast<uint8_t>(qv[0]);
    if (npx > 1) d[1] = static_cast<uint8_t>(qv[1]);
    if (npx > 2) d[2] = static_cast<uint8_t>(qv[2]);
    if (npx > 3) d[3] = static_cast<uint8_t>(qv[3]);
  }
}

// cv::invert of a 3x3 double matrix: closed form (the library's path for n <= 3)
bool invert3x3(const double *S, double *t) {
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (d == 0.) return false;
  d = 1. / d;
  t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
  t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
  t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
  t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
  t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
  t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
  t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
  return true;
}

// the per-column / per-row tables of initUndistortRectifyMap as cv::undistort calls it (stripes of 4096 / cols rows)
bool build_tables(int w, int h, const sdvl_camera *cam, double *xw, double *yw) {
  const int stripe0 = std::min(std::max(1, (1 << 12) / std::max(w, 1)), h);
  for (int y0 = 0; y0 < h; y0 += stripe0) {
    const int stripe = std::min(stripe0, h - y0);
    const double Ar[9] = {cam->fx, 0, cam->u0, 0, cam->fy, cam->v0 - y0, 0, 0, 1};
    double ir[9];
    if (!invert3x3(Ar, ir)) return false;
    for (int i = 0; i < stripe; i++) {
      double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
      // along a row _y and _w only ever receive ir[3] = ir[6] = 0, so the row's y is the value at j = 0
      yw[y0 + i] = _y * (1. / _w);
      if (y0 == 0 && i == 0)  // _x does not depend on the stripe or the row (ir[1] = 0; ir[0], ir[2] do not involve Ar(1,2))
        for (int j = 0; j < w; j++, _x += ir[0], _w += ir[6]) xw[j] = _x * (1. / _w);
    }
  }
  return true;
}

// ---- the two halves every route shares: "get the map" (the camera's, or a rectified camera's) and "remap with a map"
struct MapRef {
  const uint32_t *words;  // per-pixel words, row pitch `pitch`
  const QuadRec *quads;   // per-quad records
  int pitch;
  bool wide;              // two words per pixel
};

int map_pitch(int w) { return (w + 3) / 4 * 4; }
bool map_is_wide(int w, int h) { return w > kMapMax || h > kMapMax; }  // integer parts beyond the packed word's 11 bits: two words per pixel

// a map's allocation: per-pixel words | per-quad records, and for a rectified camera's map | the count of pixels without a source
struct MapLayout {
  sdvl_part<uint32_t> px;
  sdvl_part<QuadRec> quads;
  sdvl_part<unsigned int> count;
  size_t bytes;
  MapLayout(int w, int h, bool with_count) {
    sdvl_layout m;
    const int pitch = map_pitch(w);
    px = m.take<uint32_t>((map_is_wide(w, h) ? 2 : 1) * static_cast<size_t>(pitch) * h);
    quads = m.take<QuadRec>(static_cast<size_t>(pitch / 4) * h);
    if (with_count) count = m.take<unsigned int>(1);
    bytes = m.bytes();
  }
};

// room for a map of `bytes` in *d_map (grown only)
int map_storage(sdvl_ctx *ctx, void **d_map, size_t *have, size_t bytes) {
  if (*have >= bytes) return SDVL_OK;
  if (*d_map) {
    SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));  // remaps that read the old map may still be queued
    SDVL_HIP_CHECK(ctx, hipFree(*d_map));
    *d_map = nullptr;
    *have = 0;
  }
  SDVL_HIP_CHECK(ctx, sdvl_bind_device(ctx));
  SDVL_HIP_CHECK(ctx, hipMalloc(d_map, bytes));
  *have = bytes;
  return SDVL_OK;
}

// the per-quad records behind freshly written per-pixel words
int build_quads(sdvl_ctx *ctx, const UndistParams &P, bool wide_map, const uint32_t *d_map, QuadRec *d_quads) {
  const int pitch = map_pitch(P.w);
  if (wide_map)
    SDVL_LAUNCH(ctx, "undistort_map", undistort_quad_kernel<true>, dim3((pitch / 4 + 255) / 256, P.h), dim3(256), d_map, pitch, P, d_quads);
  else
    SDVL_LAUNCH(ctx, "undistort_map", undistort_quad_kernel<false>, dim3((pitch / 4 + 255) / 256, P.h), dim3(256), d_map, pitch, P, d_quads);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  return SDVL_OK;
}

// the camera's map: built once per (size, intrinsics, distortion, source stride) and context
int undistort_map_of(sdvl_ctx *ctx, const UndistParams &P, const sdvl_camera *cam, MapRef *out) {
  const int w = P.w, h = P.h, pitch = map_pitch(w);
  const bool wide_map = map_is_wide(w, h);
  double key[12] = {P.fx, P.fy, P.u0, P.v0, P.k1, P.k2, P.p1, P.p2, P.k3, static_cast<double>(w), static_cast<double>(h),
                    static_cast<double>(P.sstride)};  // (the quad records hold source offsets)
  const MapLayout m(w, h, false);
  if (!ctx->d_undist_map || memcmp(key, ctx->undist_key, sizeof(key)) != 0) {
    int rc = map_storage(ctx, &ctx->d_undist_map, &ctx->undist_map_bytes, m.bytes);
    if (rc) return rc;
    sdvl_layout st;  // staging: the column table | the row table
    const sdvl_part<double> st_xw = st.take<double>(w), st_yw = st.take<double>(h);
    void *hs = nullptr, *dsx = nullptr;
    rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
    if (rc) return rc;
    if (!build_tables(w, h, cam, st_xw.in(hs), st_yw.in(hs))) {
      ctx->err = "camera matrix is singular";
      return SDVL_ERR_INVALID;
    }
    SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
    const double *d_xw = st_xw.cin(dsx), *d_yw = st_yw.cin(dsx);
    uint32_t *d_map = m.px.in(ctx->d_undist_map);
    if (wide_map)
      SDVL_LAUNCH(ctx, "undistort_map", undistort_map_kernel<true>, dim3((pitch + 255) / 256, h), dim3(256), d_xw, d_yw, P, pitch, d_map);
    else
      SDVL_LAUNCH(ctx, "undistort_map", undistort_map_kernel<false>, dim3((pitch + 255) / 256, h), dim3(256), d_xw, d_yw, P, pitch, d_map);
    rc = build_quads(ctx, P, wide_map, d_map, m.quads.in(ctx->d_undist_map));
    if (rc) return rc;
    ctx->undist_quads = m.quads.in(ctx->d_undist_map);
    memcpy(ctx->undist_key, key, sizeof(key));
    ctx->undist_maps_built++;
  }
  *out = MapRef{m.px.cin(ctx->d_undist_map), static_cast<const QuadRec *>(ctx->undist_quads), pitch, wide_map};
  return SDVL_OK;
}

UndistParams rectify_params(const sdvl_rectification *r, int w, int h, int src_stride, int dst_stride) {
  return UndistParams{r->raw.fx, r->raw.fy, r->raw.u0, r->raw.v0, r->dist.d[0], r->dist.d[1], r->dist.d[2], r->dist.d[3], r->dist.d[4], w, h, src_stride, dst_stride};
}

// a rectified camera's map: looked up in the context's cache, built into its least recently used slot
int rectify_map_of(sdvl_ctx *ctx, const UndistParams &P, const sdvl_rectification *r, MapRef *out) {
  const int w = P.w, h = P.h, pitch = map_pitch(w);
  const bool wide_map = map_is_wide(w, h);
  double key[25] = {P.fx, P.fy, P.u0, P.v0, P.k1, P.k2, P.p1, P.p2, P.k3};
  for (int i = 0; i < 9; i++) key[9 + i] = r->R[i];
  key[18] = r->rect.fx, key[19] = r->rect.fy, key[20] = r->rect.u0, key[21] = r->rect.v0;
  key[22] = w, key[23] = h, key[24] = P.sstride;
  const MapLayout m(w, h, true);
  sdvl_ctx::RectMap *slot = nullptr;
  for (sdvl_ctx::RectMap &s : ctx->rect_maps)
    if (s.used && memcmp(key, s.key, sizeof(key)) == 0) slot = &s;
  if (!slot) {
    slot = &ctx->rect_maps[0];
    for (sdvl_ctx::RectMap &s : ctx->rect_maps)
      if (s.used < slot->used) slot = &s;
    slot->used = 0;  // (not a map until the build below has been queued)
    int rc = map_storage(ctx, &slot->d_map, &slot->bytes, m.bytes);
    if (rc) return rc;
    // M = R_i^T K_rect^-1, every entry as written here
    const double ifx = 1.0 / r->rect.fx, ify = 1.0 / r->rect.fy, cx = -r->rect.u0 * ifx, cy = -r->rect.v0 * ify;
    RectifyRays rays;
    for (int k = 0; k < 3; k++) {
      const double a = r->R[k], b = r->R[3 + k], c = r->R[6 + k];  // row k of R_i^T
      rays.M[3 * k] = a * ifx;
      rays.M[3 * k + 1] = b * ify;
      rays.M[3 * k + 2] = a * cx + b * cy + c;
    }
    uint32_t *d_map = m.px.in(slot->d_map);
    unsigned int *d_count = m.count.in(slot->d_map);
    SDVL_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned int), ctx->stream));
    if (wide_map)
      SDVL_LAUNCH(ctx, "rectify_map", rectify_map_kernel<true>, dim3((pitch + 255) / 256, h), dim3(256), rays, P, pitch, d_map, d_count);
    else
      SDVL_LAUNCH(ctx, "rectify_map", rectify_map_kernel<false>, dim3((pitch + 255) / 256, h), dim3(256), rays, P, pitch, d_map, d_count);
    rc = build_quads(ctx, P, wide_map, d_map, m.quads.in(slot->d_map));
    if (rc) return rc;
    // the count comes back with the build: once per camera, so the wait is not on any frame's path
    SDVL_HIP_CHECK(ctx, hipMemcpyAsync(&ctx->rect_count_host, d_count, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
    ctx->rect_no_source_last = ctx->rect_count_host;
    slot->quads = m.quads.in(slot->d_map);
    memcpy(slot->key, key, sizeof(key));
    ctx->rect_maps_built++;
  }
  slot->used = ++ctx->rect_tick;
  *out = MapRef{m.px.cin(slot->d_map), static_cast<const QuadRec *>(slot->quads), pitch, wide_map};
  return SDVL_OK;
}

// raw images in host memory go to a device scratch area first: srcs[i] and *src_stride name what the remap reads
int stage_sources(sdvl_ctx *ctx, int n, const void *const *src, int *src_stride, int src_on_device, int w, int h, std::vector<const uint8_t *> *srcs) {
  srcs->resize(n);
  if (src_on_device) {
    for (int i = 0; i < n; i++) (*srcs)[i] = static_cast<const uint8_t *>(src[i]);
    return SDVL_OK;
  }
  const size_t img_bytes = static_cast<size_t>(w) * h;
  int rc = sdvl_ensure(ctx, &ctx->d_work, &ctx->d_work_bytes, img_bytes * n, false);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    uint8_t *d = static_cast<uint8_t *>(ctx->d_work) + img_bytes * i;
    SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(d, w, src[i], *src_stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    (*srcs)[i] = d;
  }
  *src_stride = w;
  return SDVL_OK;
}

int remap_with_map(sdvl_ctx *ctx, int n, const std::vector<const uint8_t *> &srcs, uint8_t *const *dst, const UndistParams &P, const MapRef &map) {
  const size_t jb = sizeof(UndistJob) * n;
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_stage_alloc(ctx, jb, &hs, &dsx);
  if (rc) return rc;
  UndistJob *hj = static_cast<UndistJob *>(hs);
  int wide = ((P.dstride | P.w) & 3) == 0 ? 1 : 0;
  for (int i = 0; i < n; i++) {
    hj[i] = UndistJob{srcs[i], dst[i]};
    if (reinterpret_cast<uintptr_t>(dst[i]) & 3u) wide = 0;
  }
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, jb));
  const dim3 grid((n + kRemapFrames - 1) / kRemapFrames, (P.w + 127) / 128, (P.h + 7) / 8);
  if (map.wide)
    SDVL_LAUNCH(ctx, "undistort", undistort_remap_kernel<true>, grid, dim3(256), static_cast<const UndistJob *>(dsx), map.words, map.quads, map.pitch, n, wide, P);
  else
    SDVL_LAUNCH(ctx, "undistort", undistort_remap_kernel<false>, grid, dim3(256), static_cast<const UndistJob *>(dsx), map.words, map.quads, map.pitch, n, wide, P);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  return SDVL_OK;
}

int run_undistort(sdvl_ctx *ctx, int n, const void *const *src, int src_stride, int src_on_device, int w, int h, const sdvl_camera *cam,
                  const sdvl_distortion *dist, uint8_t *const *dst, int dst_stride) {
  if (dist->d[0] == 0.0) {  // Camera::SetDistortions tests d0 only (camera.cc:46): otherwise out = in.clone()
    for (int i = 0; i < n; i++)
      SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(dst[i], dst_stride, src[i], src_stride, w, h,
                                           src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return SDVL_OK;
  }
  std::vector<const uint8_t *> srcs;
  int rc = stage_sources(ctx, n, src, &src_stride, src_on_device, w, h, &srcs);
  if (rc) return rc;
  const UndistParams P{cam->fx, cam->fy, cam->u0, cam->v0, dist->d[0], dist->d[1], dist->d[2], dist->d[3], dist->d[4], w, h, src_stride, dst_stride};
  MapRef map;
  rc = undistort_map_of(ctx, P, cam, &map);
  if (rc) return rc;
  return remap_with_map(ctx, n, srcs, dst, P, map);
}

int check_rectification(sdvl_ctx *ctx, const sdvl_rectification *r) {
  bool finite = true;
  for (int i = 0; i < 9; i++) finite = finite && std::isfinite(r->R[i]);
  for (int i = 0; i < 5; i++) finite = finite && std::isfinite(r->dist.d[i]);
  for (const sdvl_camera *c : {&r->raw, &r->rect}) finite = finite && std::isfinite(c->fx) && std::isfinite(c->fy) && std::isfinite(c->u0) && std::isfinite(c->v0);
  SDVL_REQUIRE(ctx, finite, "sdvl_rectify: a value of the rectification is not finite");
  SDVL_REQUIRE(ctx, r->raw.fx > 0 && r->raw.fy > 0 && r->rect.fx > 0 && r->rect.fy > 0, "sdvl_rectify: a focal length is not positive");
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      const double dot = r->R[a] * r->R[b] + r->R[3 + a] * r->R[3 + b] + r->R[6 + a] * r->R[6 + b];
      SDVL_REQUIRE(ctx, std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-9, "sdvl_rectify: R is not a rotation (R^T R differs from I by more than 1e-9)");
    }
  return SDVL_OK;
}

// the rectified route: always a remap — the rotation and the new intrinsics move every pixel, lens or not.  The remap launch is the
// undistorted route's own
int run_rectify(sdvl_ctx *ctx, int n, const void *const *src, int src_stride, int src_on_device, int w, int h, const sdvl_rectification *r,
                uint8_t *const *dst, int dst_stride) {
  int rc = check_rectification(ctx, r);
  if (rc) return rc;
  std::vector<const uint8_t *> srcs;
  rc = stage_sources(ctx, n, src, &src_stride, src_on_device, w, h, &srcs);
  if (rc) return rc;
  const UndistParams P = rectify_params(r, w, h, src_stride, dst_stride);
  MapRef map;
  rc = rectify_map_of(ctx, P, r, &map);
  if (rc) return rc;
  return remap_with_map(ctx, n, srcs, dst, P, map);
}

// the frames of a fused upload take a new level 0: their own storage, nothing of the old image's corners
int frames_take_level0(sdvl_ctx *ctx, int n, sdvl_frame *const *frames, const void *const *src, int src_stride, std::vector<uint8_t *> *dst) {
  dst->resize(n);
  for (int i = 0; i < n; i++) {
    SDVL_REQUIRE(ctx, frames[i] && src[i], "null frame or image");
    SDVL_REQUIRE(ctx, frames[i]->width == frames[0]->width && frames[i]->height == frames[0]->height, "frames of one call share a size");
    SDVL_REQUIRE(ctx, src_stride >= frames[i]->width, "stride smaller than width");
    SDVL_REQUIRE(ctx, frames[i]->width <= kMapMaxWide && frames[i]->height <= kMapMaxWide, "image size out of range (2 .. 4095 a side)");
    frames[i]->v.level[0] = frames[i]->own_level0;
    (*dst)[i] = frames[i]->own_level0;
    frames[i]->hdr_stale = 1;
    frames[i]->v.n_corners = 0;
    frames[i]->desc_valid = 0;
    frames[i]->bins_valid = 0;
  }
  return SDVL_OK;
}

}  // namespace

extern "C" {

int sdvl_undistort(sdvl_ctx *ctx, int n, const void *const *src, int src_stride, int src_on_device, int width, int height,
                   const sdvl_camera *cam, const sdvl_distortion *dist, void *const *dst_dev, int dst_stride) {
  if (!ctx || n < 0 || (n > 0 && (!src || !dst_dev)) || !cam || !dist) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, width >= 2 && height >= 2 && width <= kMapMaxWide && height <= kMapMaxWide, "image size out of range (2 .. 4095 a side)");
  SDVL_REQUIRE(ctx, src_stride >= width && dst_stride >= width, "stride smaller than width");
  for (int i = 0; i < n; i++) SDVL_REQUIRE(ctx, src[i] && dst_dev[i] && src[i] != dst_dev[i], "null image or in-place undistort");
  return run_undistort(ctx, n, src, src_stride, src_on_device, width, height, cam, dist, reinterpret_cast<uint8_t *const *>(dst_dev), dst_stride);
}

int sdvl_frames_upload_undistorted(sdvl_ctx *ctx, int n, sdvl_frame *const *frames, const void *const *src, int src_stride,
                                   int src_on_device, const sdvl_camera *cam, const sdvl_distortion *dist) {
  if (!ctx || n < 0 || (n > 0 && (!frames || !src)) || !cam || !dist) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  std::vector<uint8_t *> dst;
  const int rc = frames_take_level0(ctx, n, frames, src, src_stride, &dst);
  if (rc) return rc;
  return run_undistort(ctx, n, src, src_stride, src_on_device, frames[0]->width, frames[0]->height, cam, dist, dst.data(), frames[0]->width);
}

int sdvl_rectify(sdvl_ctx *ctx, int n, const void *const *src, int src_stride, int src_on_device, int width, int height,
                 const sdvl_rectification *r, void *const *dst_dev, int dst_stride) {
  if (!ctx || n < 0 || (n > 0 && (!src || !dst_dev)) || !r) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, width >= 2 && height >= 2 && width <= kMapMaxWide && height <= kMapMaxWide, "image size out of range (2 .. 4095 a side)");
  SDVL_REQUIRE(ctx, src_stride >= width && dst_stride >= width, "stride smaller than width");
  for (int i = 0; i < n; i++) SDVL_REQUIRE(ctx, src[i] && dst_dev[i] && src[i] != dst_dev[i], "null image or in-place rectification");
  return run_rectify(ctx, n, src, src_stride, src_on_device, width, height, r, reinterpret_cast<uint8_t *const *>(dst_dev), dst_stride);
}

int sdvl_frames_upload_rectified(sdvl_ctx *ctx, int n, sdvl_frame *const *frames, const void *const *src, int src_stride,
                                 int src_on_device, const sdvl_rectification *r) {
  if (!ctx || n < 0 || (n > 0 && (!frames || !src)) || !r) return SDVL_ERR_INVALID;
  if (n == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, frames[0] && frames[0]->width >= 2 && frames[0]->height >= 2, "null frame or image");
  std::vector<uint8_t *> dst;
  const int rc = frames_take_level0(ctx, n, frames, src, src_stride, &dst);
  if (rc) return rc;
  return run_rectify(ctx, n, src, src_stride, src_on_device, frames[0]->width, frames[0]->height, r, dst.data(), frames[0]->width);
}

int sdvl_rectify_stats(sdvl_ctx *ctx, int64_t *out2) {
  if (!ctx || !out2) return SDVL_ERR_INVALID;
  out2[0] = ctx->rect_maps_built;
  out2[1] = ctx->rect_no_source_last;
  return SDVL_OK;
}

int sdvl_rectify_map_words(sdvl_ctx *ctx, int width, int height, int src_stride, const sdvl_rectification *r, uint32_t *out_words) {
  if (!ctx || !r || !out_words) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, width >= 2 && height >= 2 && width <= kMapMaxWide && height <= kMapMaxWide, "image size out of range (2 .. 4095 a side)");
  SDVL_REQUIRE(ctx, src_stride >= width, "stride smaller than width");
  int rc = check_rectification(ctx, r);
  if (rc) return rc;
  MapRef map;
  rc = rectify_map_of(ctx, rectify_params(r, width, height, src_stride, width), r, &map);
  if (rc) return rc;
  const size_t word_bytes = (map.wide ? 2 : 1) * sizeof(uint32_t);
  SDVL_HIP_CHECK(ctx, hipMemcpy2DAsync(out_words, width * word_bytes, map.words, map.pitch * word_bytes, width * word_bytes, height, hipMemcpyDeviceToHost, ctx->stream));
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  return SDVL_OK;
}

}  // extern "C"
