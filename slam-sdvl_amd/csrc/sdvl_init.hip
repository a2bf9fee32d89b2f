// sdvl_init.hip — the two OpenCV calls of the reference's two-frame initialisation (homography_init.cc:185-282) on the device:
//   sdvl_klt_track          cv::calcOpticalFlowPyrLK(prev, next, pixels1_, pixels2_, ..., Size(30, 30), 4, (30, 0.001),
//                           OPTFLOW_USE_INITIAL_FLOW), :195-198
//   sdvl_homography_ransac  the RANSAC loop of cv::findHomography(src, dst, CV_RANSAC, 2 / fx), :253
// Neither is pinned to OpenCV's bits (it is no dependency of this project): tests/klt_restatement.py and
// tests/homography_restatement.py state what is computed, DESIGN §2 what differs from OpenCV.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "sdvl_internal.h"
#include "sdvl_wave.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- KLT
constexpr int kWin = 30, kWinArea = kWin * kWin;
constexpr int kSlots = (kWinArea + 63) / 64;  // window pixels per lane: 15 (the last slot is live in lanes 0..3 only)

struct KltJobDev {
  FrameView prev, next;
};

struct KltParamsDev {
  int max_level, max_its;
  double eps2, min_eig_threshold;
};

// every read clamps to the level's edge: no coordinate, however wild, leaves the image
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct Weights {
  float w00, w01, w10, w11;
};

__device__ __forceinline__ Weights bilinear_weights(float a, float b) {
  Weights w;
  w.w00 = (1.0f - a) * (1.0f - b);
  w.w01 = a * (1.0f - b);
  w.w10 = (1.0f - a) * b;
  w.w11 = 1.0f - w.w00 - w.w01 - w.w10;
  return w;
}

__device__ __forceinline__ float mix4(float v00, float v01, float v10, float v11, const Weights &w) {
  return ((v00 * w.w00 + v01 * w.w01) + v10 * w.w10) + v11 * w.w11;
}

// the level image at (x0, y0) .. (x0 + 1, y0 + 1)
__device__ __forceinline__ float sample_u8(const uint8_t *__restrict__ img, int lw, int lh, int x0, int y0, const Weights &w) {
  const int xa = clampi(x0, lw - 1), xb = clampi(x0 + 1, lw - 1);
  const uint8_t *ra = img + static_cast<size_t>(clampi(y0, lh - 1)) * lw, *rb = img + static_cast<size_t>(clampi(y0 + 1, lh - 1)) * lw;
  return mix4(ra[xa], ra[xb], rb[xa], rb[xb], w);
}

// float -> int the way every caller below needs it: floor, NaN -> 0, saturating — spelled out, so that no conversion is undefined
__device__ __forceinline__ int floor_int(float v) {
  v = floorf(v);
  if (!(v == v)) return 0;
  return static_cast<int>(fminf(fmaxf(v, -2147483648.0f), 2147483520.0f));
}

__device__ __forceinline__ bool window_inside(int ix, int iy, int lw, int lh) { return ix >= -kWin && ix < lw && iy >= -kWin && iy < lh; }

// One wave per point.  Lane l owns window pixels l, l + 64, ...: their template value and Scharr gradients stay in registers for the
// level's iterations; the sums over the window are wave reductions.
__global__ __launch_bounds__(64) void klt_track_kernel(const KltJobDev *__restrict__ jobs, const int32_t *__restrict__ pt_job,
                                                       const float *__restrict__ prev_xy, float *__restrict__ next_xy,
                                                       uint8_t *__restrict__ status, float *__restrict__ err, int n_pts, KltParamsDev prm) {
  const int pt = blockIdx.x, lane = threadIdx.x;
  if (pt >= n_pts) return;
  const int j = pt_job[pt];
  if (j < 0) {  // a point of no job
    if (lane == 0) {
      status[pt] = 0;
      err[pt] = 0.0f;
    }
    return;
  }
  const FrameView &fp = jobs[j].prev, &fn = jobs[j].next;
  const float half = (kWin - 1) * 0.5f;
  const float prev_x = prev_xy[2 * pt], prev_y = prev_xy[2 * pt + 1];
  float out_x = next_xy[2 * pt], out_y = next_xy[2 * pt + 1];
  bool alive = true;
  float tI[kSlots], tIx[kSlots], tIy[kSlots];
  for (int level = prm.max_level; level >= 0; level--) {
    const int lw = fp.lw[level], lh = fp.lh[level];
    const uint8_t *__restrict__ I = fp.level[level], *__restrict__ J = fn.level[level];
    const float scale = 1.0f / static_cast<float>(1 << level);
    if (level == prm.max_level) {
      out_x *= scale;
      out_y *= scale;
    } else {
      out_x *= 2.0f;
      out_y *= 2.0f;
    }
    const float px = prev_x * scale - half, py = prev_y * scale - half;
    const int ipx = floor_int(px), ipy = floor_int(py);
    if (!window_inside(ipx, ipy, lw, lh)) {
      if (level == 0) alive = false;
      continue;
    }
    const Weights wp = bilinear_weights(px - static_cast<float>(ipx), py - static_cast<float>(ipy));
    float a11 = 0.0f, a12 = 0.0f, a22 = 0.0f;
#pragma unroll
    for (int k = 0; k < kSlots; k++) {
      const int idx = lane + 64 * k;
      const int wy = idx / kWin, wx = idx - wy * kWin;
      const int x0 = ipx + wx, y0 = ipy + wy;
      // the 4x4 block around the sample: Scharr (3, 10, 3) / 32 at its four inner pixels, clamped reads
      int p[4][4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint8_t *row = I + static_cast<size_t>(clampi(y0 - 1 + r, lh - 1)) * lw;
#pragma unroll
        for (int c = 0; c < 4; c++) p[r][c] = row[clampi(x0 - 1 + c, lw - 1)];
      }
      float gx[2][2], gy[2][2];
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
          const int sx = 3 * (p[r][c + 2] - p[r][c]) + 10 * (p[r + 1][c + 2] - p[r + 1][c]) + 3 * (p[r + 2][c + 2] - p[r + 2][c]);
          const int sy = 3 * (p[r + 2][c] - p[r][c]) + 10 * (p[r + 2][c + 1] - p[r][c + 1]) + 3 * (p[r + 2][c + 2] - p[r][c + 2]);
          gx[r][c] = static_cast<float>(sx) * (1.0f / 32.0f);
          gy[r][c] = static_cast<float>(sy) * (1.0f / 32.0f);
        }
      const bool live = idx < kWinArea;
      const float vi = mix4(p[1][1], p[1][2], p[2][1], p[2][2], wp);
      const float vx = mix4(gx[0][0], gx[0][1], gx[1][0], gx[1][1], wp);
      const float vy = mix4(gy[0][0], gy[0][1], gy[1][0], gy[1][1], wp);
      tI[k] = live ? vi : 0.0f;
      tIx[k] = live ? vx : 0.0f;
      tIy[k] = live ? vy : 0.0f;
      a11 += tIx[k] * tIx[k];
      a12 += tIx[k] * tIy[k];
      a22 += tIy[k] * tIy[k];
    }
    // OpenCV's units: its template and gradients are 32-fold, its sums carry FLT_SCALE = 2^-20
    const float A11 = wave_sum_dpp_f32(a11) * (1.0f / 1024.0f), A12 = wave_sum_dpp_f32(a12) * (1.0f / 1024.0f), A22 = wave_sum_dpp_f32(a22) * (1.0f / 1024.0f);
    float D = A11 * A22 - A12 * A12;
    const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.0f * A12 * A12)) / static_cast<float>(2 * kWinArea);
    if (static_cast<double>(min_eig) < prm.min_eig_threshold || D < FLT_EPSILON) {
      if (level == 0) alive = false;
      continue;
    }
    D = 1.0f / D;
    float nx = out_x - half, ny = out_y - half;
    float pdx = 0.0f, pdy = 0.0f;
    for (int it = 0; it < prm.max_its; it++) {
      const int inx = floor_int(nx), iny = floor_int(ny);
      if (!window_inside(inx, iny, lw, lh)) {
        if (level == 0) alive = false;
        break;
      }
      const Weights wn = bilinear_weights(nx - static_cast<float>(inx), ny - static_cast<float>(iny));
      float b1 = 0.0f, b2 = 0.0f;
#pragma unroll
      for (int k = 0; k < kSlots; k++) {
        const int idx = lane + 64 * k;
        const int wy = idx / kWin, wx = idx - wy * kWin;
        const float diff = sample_u8(J, lw, lh, inx + wx, iny + wy, wn) - tI[k];
        b1 += diff * tIx[k];  // a dead slot has zero gradients
        b2 += diff * tIy[k];
      }
      const float B1 = wave_sum_dpp_f32(b1) * (1.0f / 1024.0f), B2 = wave_sum_dpp_f32(b2) * (1.0f / 1024.0f);
      const float dx = (A12 * B2 - A22 * B1) * D, dy = (A12 * B1 - A11 * B2) * D;
      nx += dx;
      ny += dy;
      out_x = nx + half;
      out_y = ny + half;
      if (static_cast<double>(dx) * static_cast<double>(dx) + static_cast<double>(dy) * static_cast<double>(dy) <= prm.eps2) break;
      if (it > 0 && static_cast<double>(fabsf(dx + pdx)) < 0.01 && static_cast<double>(fabsf(dy + pdy)) < 0.01) {
        out_x -= dx * 0.5f;
        out_y -= dy * 0.5f;
        break;
      }
      pdx = dx;
      pdy = dy;
    }
  }
  // a result outside the image is lost (NaN compares false)
  const int w0 = fp.lw[0], h0 = fp.lh[0];
  alive = alive && out_x >= 0.0f && out_x < static_cast<float>(w0) && out_y >= 0.0f && out_y < static_cast<float>(h0);
  // err: mean absolute difference of the window at the result; tI still holds the level-0 template when the point is alive
  float e = 0.0f;
  if (alive) {
    const float nx = out_x - half, ny = out_y - half;
    const int inx = floor_int(nx), iny = floor_int(ny);
    const Weights wn = bilinear_weights(nx - static_cast<float>(inx), ny - static_cast<float>(iny));
#pragma unroll
    for (int k = 0; k < kSlots; k++) {
      const int idx = lane + 64 * k;
      const int wy = idx / kWin, wx = idx - wy * kWin;
      if (idx < kWinArea) e += fabsf(sample_u8(fn.level[0], w0, h0, inx + wx, iny + wy, wn) - tI[k]);
    }
  }
  e = wave_sum_dpp_f32(e) / static_cast<float>(kWinArea);
  if (lane == 0) {
    next_xy[2 * pt] = out_x;
    next_xy[2 * pt + 1] = out_y;
    status[pt] = alive ? 1 : 0;
    err[pt] = e;
  }
}

// ------------------------------------------------------------------------------------------------- homography RANSAC
constexpr int kMaxMatches = SDVL_MAX_LEVEL_CELLS;

struct HomJobDev {
  int m_begin, n_m;
  int draw_begin, n_draws;  // n_draws: already limited to max_its
  int nits_begin, pad_;
};

struct Hom3 {
  double h[9];
};

__device__ __forceinline__ bool collinear3(const double *x, const double *y, int i, int j, int k) {
  const double dx1 = x[j] - x[i], dy1 = y[j] - y[i], dx2 = x[k] - x[i], dy2 = y[k] - y[i];
  return fabs(dx2 * dy1 - dy2 * dx1) <= static_cast<double>(FLT_EPSILON) * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

// adj(M) of M = [p1 p2 p3] (homogeneous columns) and lambda' = adj(M) p4
__device__ __forceinline__ void adj_lambda(const double *x, const double *y, double adj[3][3], double lam[3]) {
  adj[0][0] = y[1] - y[2]; adj[0][1] = x[2] - x[1]; adj[0][2] = x[1] * y[2] - x[2] * y[1];
  adj[1][0] = y[2] - y[0]; adj[1][1] = x[0] - x[2]; adj[1][2] = x[2] * y[0] - x[0] * y[2];
  adj[2][0] = y[0] - y[1]; adj[2][1] = x[1] - x[0]; adj[2][2] = x[0] * y[1] - x[1] * y[0];
  for (int i = 0; i < 3; i++) lam[i] = (adj[i][0] * x[3] + adj[i][1] * y[3]) + adj[i][2];
}

// H of the draw's four correspondences; false: repeated index or three collinear points (no model)
__device__ bool homography_of_draw(const double2 *__restrict__ src, const double2 *__restrict__ dst, int n_m, const int32_t *__restrict__ d4, Hom3 *H) {
  int id[4];
  for (int i = 0; i < 4; i++) {
    id[i] = d4[i];
    if (id[i] < 0 || id[i] >= n_m) return false;  // checked on the host already; never index outside the job
  }
  if (id[0] == id[1] || id[0] == id[2] || id[0] == id[3] || id[1] == id[2] || id[1] == id[3] || id[2] == id[3]) return false;
  double sx[4], sy[4], dx[4], dy[4];
  for (int i = 0; i < 4; i++) {
    const double2 s = src[id[i]], d = dst[id[i]];
    sx[i] = s.x; sy[i] = s.y; dx[i] = d.x; dy[i] = d.y;
  }
  if (collinear3(sx, sy, 0, 1, 2) || collinear3(dx, dy, 0, 1, 2) || collinear3(sx, sy, 0, 1, 3) || collinear3(dx, dy, 0, 1, 3) ||
      collinear3(sx, sy, 0, 2, 3) || collinear3(dx, dy, 0, 2, 3) || collinear3(sx, sy, 1, 2, 3) || collinear3(dx, dy, 1, 2, 3))
    return false;
  double adj[3][3], lam[3], adj_d[3][3], mu[3];
  adj_lambda(sx, sy, adj, lam);
  adj_lambda(dx, dy, adj_d, mu);
  const double sc[3] = {mu[0] / lam[0], mu[1] / lam[1], mu[2] / lam[2]};
  const double N[3][3] = {{dx[0], dx[1], dx[2]}, {dy[0], dy[1], dy[2]}, {1.0, 1.0, 1.0}};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) H->h[3 * r + c] = ((N[r][0] * sc[0]) * adj[0][c] + (N[r][1] * sc[1]) * adj[1][c]) + (N[r][2] * sc[2]) * adj[2][c];
  if (fabs(H->h[8]) > DBL_EPSILON) {
    const double inv = 1.0 / H->h[8];
    for (int i = 0; i < 9; i++) H->h[i] = H->h[i] * inv;
  }
  return true;
}

__device__ __forceinline__ bool supports(const Hom3 &H, const double2 s, const double2 d, double t2) {
  const double w = (H.h[6] * s.x + H.h[7] * s.y) + H.h[8];
  const double ex = ((H.h[0] * s.x + H.h[1] * s.y) + H.h[2]) / w - d.x;
  const double ey = ((H.h[3] * s.x + H.h[4] * s.y) + H.h[5]) / w - d.y;
  return ex * ex + ey * ey <= t2;  // NaN (w == 0) supports nothing
}

// lane per draw: the support of every draw the sequential loop could reach; -1 = no model
__global__ __launch_bounds__(64) void homography_hypotheses_kernel(const HomJobDev *__restrict__ jobs, const double2 *__restrict__ src,
                                                                   const double2 *__restrict__ dst, const int32_t *__restrict__ draws4,
                                                                   double t2, int32_t *__restrict__ counts) {
  const HomJobDev job = jobs[blockIdx.y];
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= job.n_draws) return;
  const double2 *s = src + job.m_begin, *d = dst + job.m_begin;
  Hom3 H;
  int count = -1;
  if (homography_of_draw(s, d, job.n_m, draws4 + 4 * static_cast<size_t>(job.draw_begin + k), &H)) {
    count = 0;
    for (int m = 0; m < job.n_m; m++) count += supports(H, s[m], d[m], t2) ? 1 : 0;
  }
  counts[job.draw_begin + k] = count;
}

// one wave per job: the sequential walk over the counts (lane 0), then the best draw's inliers in ascending order
__global__ __launch_bounds__(64) void homography_select_kernel(const HomJobDev *__restrict__ jobs, const double2 *__restrict__ src,
                                                               const double2 *__restrict__ dst, const int32_t *__restrict__ draws4,
                                                               const int32_t *__restrict__ counts, const int32_t *__restrict__ nits, double t2,
                                                               sdvl_homography_result *__restrict__ results, int32_t *__restrict__ lists) {
  const HomJobDev job = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  int best = -1, it = 0;
  if (lane == 0) {
    int budget = job.n_draws, best_count = 3;
    while (it < budget) {
      const int c = counts[job.draw_begin + it];
      it++;
      if (c > best_count) {
        best = it - 1;
        best_count = c;
        budget = min(budget, nits[job.nits_begin + c]);
      }
    }
  }
  best = __builtin_amdgcn_readfirstlane(best);
  it = __builtin_amdgcn_readfirstlane(it);
  const double2 *s = src + job.m_begin, *d = dst + job.m_begin;
  sdvl_homography_result res;
  for (int i = 0; i < 9; i++) res.H[i] = 0.0;
  res.best_draw = best;
  res.n_its = it;
  res.n_inliers = 0;
  res.pad_ = 0;
  Hom3 H;
  if (best >= 0 && homography_of_draw(s, d, job.n_m, draws4 + 4 * static_cast<size_t>(job.draw_begin + best), &H)) {
    int n_in = 0;
    for (int base = 0; base < job.n_m; base += 64) {
      const int m = base + lane;
      const bool in = m < job.n_m && supports(H, s[m], d[m], t2);
      const unsigned long long mask = __ballot(in);
      if (in) lists[job.m_begin + n_in + __popcll(mask & ((1ull << lane) - 1ull))] = m;
      n_in += __popcll(mask);
    }
    res.n_inliers = n_in;
    for (int i = 0; i < 9; i++) res.H[i] = H.h[i];
  }
  if (lane == 0) results[blockIdx.x] = res;
}

// RANSACUpdateNumIters(confidence, (n - s) / n, 4, max_its) for s = 0 .. n: the budget after an improvement to s supporters
void budget_table(int n, double confidence, int max_its, int32_t *out) {
  const double p = std::min(std::max(confidence, 0.0), 1.0);
  const double num = log(std::max(1.0 - p, DBL_MIN));
  for (int s = 0; s <= n; s++) {
    const double ep = std::min(std::max(static_cast<double>(n - s) / static_cast<double>(n), 0.0), 1.0);
    double denom = 1.0 - pow(1.0 - ep, 4);
    if (denom < DBL_MIN) {
      out[s] = 0;
      continue;
    }
    denom = log(denom);
    out[s] = (denom >= 0 || -num >= max_its * (-denom)) ? max_its : static_cast<int32_t>(rint(num / denom));
  }
}

}  // namespace

extern "C" int sdvl_klt_track(sdvl_ctx *ctx, int n_jobs, const sdvl_klt_job *jobs, int n_pts, const float *prev_xy, float *next_xy,
                              uint8_t *status, float *err, const sdvl_klt_params *params) {
  if (!ctx || !params || n_jobs < 0 || n_pts < 0 || (n_jobs > 0 && !jobs) || (n_pts > 0 && (!prev_xy || !next_xy || !status))) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, params->win_size == kWin, "only win_size 30 is supported (a lane owns 15 of the 900 window pixels)");
  SDVL_REQUIRE(ctx, params->max_level >= 0 && params->max_level < SDVL_MAX_LEVELS && params->max_its >= 0 && params->max_its <= 1000, "bad max_level / max_its");
  SDVL_REQUIRE(ctx, params->eps >= 0.0 && params->min_eig_threshold == params->min_eig_threshold, "bad eps / min_eig_threshold");
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_klt_job &a = jobs[j];
    SDVL_REQUIRE(ctx, a.prev && a.next && a.prev->home == ctx && a.next->home == ctx, "frames of a job must be created on this context");
    SDVL_REQUIRE(ctx, a.prev->width == a.next->width && a.prev->height == a.next->height && a.prev->v.levels == a.next->v.levels,
                 "the two frames of a job differ in size");
    SDVL_REQUIRE(ctx, params->max_level < a.prev->v.levels, "max_level reaches beyond the frames' pyramids");
    SDVL_REQUIRE(ctx, a.pt_begin >= 0 && a.pt_end >= a.pt_begin && a.pt_end <= n_pts, "point range out of bounds");
  }
  if (n_pts == 0) return SDVL_OK;
  sdvl_layout st, o;  // staging: jobs | job of every point | prev | next ; d_out and h_out: next | err | status
  const sdvl_part<KltJobDev> st_jobs = st.take<KltJobDev>(std::max(n_jobs, 1));
  const sdvl_part<int32_t> st_ptjob = st.take<int32_t>(n_pts);
  const sdvl_part<float> st_prev = st.take<float>(2 * static_cast<size_t>(n_pts)), st_next = st.take<float>(2 * static_cast<size_t>(n_pts));
  const sdvl_part<float> o_next = o.take<float>(2 * static_cast<size_t>(n_pts)), o_err = o.take<float>(n_pts);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n_pts);
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_ensure(ctx, &ctx->d_out, &ctx->d_out_bytes, o.bytes(), false);
  if (!rc) rc = sdvl_ensure(ctx, &ctx->h_out, &ctx->h_out_bytes, o.bytes(), true);
  if (!rc) rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
  if (rc) return rc;
  int32_t *pj = st_ptjob.in(hs);
  for (int k = 0; k < n_pts; k++) pj[k] = -1;
  KltJobDev *hj = st_jobs.in(hs);
  for (int j = 0; j < n_jobs; j++) {
    hj[j].prev = jobs[j].prev->v;
    hj[j].next = jobs[j].next->v;
    for (int k = jobs[j].pt_begin; k < jobs[j].pt_end; k++) {
      SDVL_REQUIRE(ctx, pj[k] < 0, "point ranges of two jobs overlap");
      pj[k] = j;
    }
  }
  memcpy(st_prev.in(hs), prev_xy, st_prev.bytes());
  memcpy(st_next.in(hs), next_xy, st_next.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
  // the kernel updates the flow in place in d_out: seed it from the staged copy
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(o_next.in(ctx->d_out), st_next.cin(dsx), o_next.bytes(), hipMemcpyDeviceToDevice, ctx->stream));
  const KltParamsDev prm = {params->max_level, params->max_its, params->eps * params->eps, params->min_eig_threshold};
  SDVL_LAUNCH(ctx, "klt_track", klt_track_kernel, dim3(n_pts), dim3(64), st_jobs.cin(dsx), st_ptjob.cin(dsx), st_prev.cin(dsx), o_next.in(ctx->d_out),
              o_status.in(ctx->d_out), o_err.in(ctx->d_out), n_pts, prm);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, o.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  memcpy(next_xy, o_next.in(ctx->h_out), o_next.bytes());
  memcpy(status, o_status.in(ctx->h_out), o_status.bytes());
  if (err) memcpy(err, o_err.in(ctx->h_out), o_err.bytes());
  return SDVL_OK;
}

extern "C" int sdvl_homography_ransac(sdvl_ctx *ctx, int n_jobs, const sdvl_homography_job *jobs, int n_m, const double *src_xy,
                                      const double *dst_xy, int n_draws, const int32_t *draws4, double threshold, int max_its, double confidence,
                                      sdvl_homography_result *results, int32_t *inlier_lists) {
  if (!ctx || n_jobs < 0 || n_m < 0 || n_draws < 0 || (n_jobs > 0 && (!jobs || !results)) || (n_m > 0 && (!src_xy || !dst_xy || !inlier_lists)) ||
      (n_draws > 0 && !draws4))
    return SDVL_ERR_INVALID;
  if (n_jobs == 0) return SDVL_OK;
  SDVL_REQUIRE(ctx, threshold >= 0.0 && max_its >= 0 && max_its <= (1 << 20) && confidence == confidence, "bad threshold / max_its / confidence");
  size_t n_nits = 0;
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_homography_job &a = jobs[j];
    SDVL_REQUIRE(ctx, a.m_begin >= 0 && a.m_end >= a.m_begin && a.m_end <= n_m, "match range out of bounds");
    SDVL_REQUIRE(ctx, a.draw_begin >= 0 && a.draw_end >= a.draw_begin && a.draw_end <= n_draws, "draw range out of bounds");
    const int size = a.m_end - a.m_begin;
    if (size > kMaxMatches) {
      ctx->err = "too many matches in one homography job for the device path (8192)";
      return SDVL_ERR_CAPACITY;
    }
    const int walked = std::min(max_its, a.draw_end - a.draw_begin);
    for (int k = 0; k < walked; k++)
      for (int c = 0; c < 4; c++) {
        const int32_t v = draws4[4 * static_cast<size_t>(a.draw_begin + k) + c];
        SDVL_REQUIRE(ctx, v >= 0 && v < std::max(size, 1), "draw index outside the match list");
      }
    n_nits += static_cast<size_t>(size) + 1;
  }
  sdvl_layout st, o, wk;  // staging: jobs | src | dst | draws | budgets ; d_out and h_out: results | lists ; d_work: the draws' supports
  const sdvl_part<HomJobDev> st_jobs = st.take<HomJobDev>(n_jobs);
  const sdvl_part<double> st_src = st.take<double>(2 * static_cast<size_t>(n_m)), st_dst = st.take<double>(2 * static_cast<size_t>(n_m));
  const sdvl_part<int32_t> st_draws = st.take<int32_t>(4 * static_cast<size_t>(n_draws)), st_nits = st.take<int32_t>(n_nits);
  const sdvl_part<sdvl_homography_result> o_res = o.take<sdvl_homography_result>(n_jobs);
  const sdvl_part<int32_t> o_lists = o.take<int32_t>(n_m);
  const sdvl_part<int32_t> wk_counts = wk.take<int32_t>(std::max(n_draws, 1));
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_ensure(ctx, &ctx->d_work, &ctx->d_work_bytes, wk.bytes(), false);
  if (!rc) rc = sdvl_ensure(ctx, &ctx->d_out, &ctx->d_out_bytes, o.bytes(), false);
  if (!rc) rc = sdvl_ensure(ctx, &ctx->h_out, &ctx->h_out_bytes, o.bytes(), true);
  if (!rc) rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
  if (rc) return rc;
  HomJobDev *hj = st_jobs.in(hs);
  int32_t *nits = st_nits.in(hs);
  int max_walk = 0, nits_at = 0;
  for (int j = 0; j < n_jobs; j++) {
    const int size = jobs[j].m_end - jobs[j].m_begin;
    hj[j] = HomJobDev{jobs[j].m_begin, size, jobs[j].draw_begin, std::min(max_its, jobs[j].draw_end - jobs[j].draw_begin), nits_at, 0};
    if (size > 0) budget_table(size, confidence, max_its, nits + nits_at);
    else nits[nits_at] = 0;
    nits_at += size + 1;
    max_walk = std::max(max_walk, hj[j].n_draws);
  }
  if (n_m) {
    memcpy(st_src.in(hs), src_xy, st_src.bytes());
    memcpy(st_dst.in(hs), dst_xy, st_dst.bytes());
  }
  if (n_draws) memcpy(st_draws.in(hs), draws4, st_draws.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
  const double t2 = threshold * threshold;
  const double2 *d_src = reinterpret_cast<const double2 *>(st_src.cin(dsx)), *d_dst = reinterpret_cast<const double2 *>(st_dst.cin(dsx));
  int32_t *d_counts = wk_counts.in(ctx->d_work);
  if (max_walk > 0)
    SDVL_LAUNCH(ctx, "homography_hypotheses", homography_hypotheses_kernel, dim3((max_walk + 63) / 64, n_jobs), dim3(64), st_jobs.cin(dsx), d_src, d_dst,
                st_draws.cin(dsx), t2, d_counts);
  SDVL_LAUNCH(ctx, "homography_select", homography_select_kernel, dim3(n_jobs), dim3(64), st_jobs.cin(dsx), d_src, d_dst, st_draws.cin(dsx),
              static_cast<const int32_t *>(d_counts), st_nits.cin(dsx), t2, o_res.in(ctx->d_out), o_lists.in(ctx->d_out));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, o.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  memcpy(results, o_res.in(ctx->h_out), o_res.bytes());
  if (n_m) memcpy(inlier_lists, o_lists.in(ctx->h_out), o_lists.bytes());
  return SDVL_OK;
}
