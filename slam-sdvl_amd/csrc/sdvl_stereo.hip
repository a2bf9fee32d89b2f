// sdvl_stereo.hip — stereo cameras: the depth of a keyframe's filtered corners from a rectified right image (sdvl_stereo_depth), the
// producer of the `z` / `status` contract that sdvl_depth_seed fills for a depth camera.  A sparse matcher: costs are taken at the
// corners only, never a dense disparity image.  The rule is this project's own and tests/stereo_restatement.py is its specification:
//   window    the 9 x 9 samples at (X + i s, Y + j s), i, j in -4 .. 4, (X, Y) = (x << l, y << l), s = 1 << l, of level 0 of both images
//   range     d_lo = floor(fx b / max_depth) (no max_depth: 0), d_hi = min(max_disparity, floor(fx b / min_depth), X - 4 s)
//   cost      S(d) = sum |L - R| over the 81 samples, an integer <= 20 655; d0 its argmin, ties to the smallest d; four half-window costs
//             from the same absolute differences (sample columns 0-4, 4-8, rows 0-4, 4-8)
//   status    the first that applies of OUTSIDE (left window off the image, fewer than 3 disparities), NOMATCH (S(d0) > 81 max_sad, d0 an
//             end of the range), AMBIGUOUS (100 S(d0) > uniqueness S2, S2 = min S(d) over |d - d0| > 1), EDGE (a half window's argmin
//             differs from d0 by more than 1); otherwise OK
//   result    delta = 0.5 (S- - S+) / (S- - 2 S0 + S+) (denominator > 0, else 0), disparity = d0 + delta, z = fx b / disparity
// stereo_depth: one wave per corner, lane per disparity (d_lo + lane + 64 k, at most 8 rounds).  The wave stages the right strip — 9 rows
// x (range + 8 s) bytes — and the 81 left samples in LDS; a lane sums its 81 absolute differences into nine accumulators (sample columns
// < 4, = 4, > 4 times rows alike), from which the full and the four half-window costs are sums.  The five argmins are 32-bit minima over
// keys S 512 + index (wave_min_u32: DPP steps); the costs go to LDS, from which S2, S- and S+ are read.  No floating point before the
// parabola, which one lane evaluates in double, in the restatement's operation order (-ffp-contract=off).
#include <string>

#include "sdvl_depth_device.h"
#include "sdvl_wave.h"

namespace {

constexpr int kHalf = 4, kSide = 2 * kHalf + 1;   // the window
constexpr int kMaxRange = 512;                    // disparities 0 .. 511: 8 rounds of 64 lanes
constexpr int kLeftBytes = 96;                    // 81 left samples, padded
constexpr uint32_t kNoKey = 0xffffffffu;

struct StereoJobDev {
  const uint8_t *left;   // level 0 of the left frame
  const uint8_t *right;  // device-visible address of the right image
  int32_t lstride, rstride;
  int32_t width, height;
};

struct StereoRule {
  double fb;  // fx x baseline
  int32_t d_lo, d_cap;
  int32_t max_cost;  // 81 x max_sad
  int32_t uniqueness;
};

// one row of a window: the nine absolute differences into the sums of sample columns < 4, = 4, > 4
__device__ __forceinline__ void row_sad(const uint8_t *l, const uint8_t *r, int s, uint32_t g[3]) {
#pragma unroll
  for (int i = 0; i < kSide; i++) {
    const int a = l[i], b = r[i * s];
    g[i < kHalf ? 0 : i == kHalf ? 1 : 2] += static_cast<uint32_t>(a > b ? a - b : b - a);
  }
}

// Dynamic LDS of the block (one wave): cost[512] uint32 | left[96] | strip[9][sw_max]
__global__ __launch_bounds__(64) void stereo_depth(const StereoJobDev *__restrict__ jobs, const int32_t *__restrict__ xyl,
                                                   const int32_t *__restrict__ corner_job, StereoRule rule, int sw_max,
                                                   double *__restrict__ out_z, double *__restrict__ out_disparity,
                                                   uint8_t *__restrict__ out_status) {
  extern __shared__ uint32_t lds[];
  uint32_t *cost = lds;
  uint8_t *left = reinterpret_cast<uint8_t *>(lds + kMaxRange);
  uint8_t *strip = left + kLeftBytes;
  const int c = blockIdx.x, lane = threadIdx.x;
  const int jb = corner_job[c];
  int status = SDVL_STEREO_NOMATCH;  // a corner no job names
  double disparity = 0.0, z = 0.0;
  // every condition up to the lanes' own disparities is the same in all lanes: the wave leaves the branches together
  if (jb >= 0) {
    const StereoJobDev job = jobs[jb];
    const int x = xyl[3 * c], y = xyl[3 * c + 1], s = 1 << xyl[3 * c + 2];
    status = SDVL_STEREO_OUTSIDE;
    // (x, y < 16384 before they are scaled: no overflow)
    const bool inside = x >= 0 && y >= 0 && x < job.width && y < job.height && x * s - kHalf * s >= 0 && x * s + kHalf * s < job.width &&
                        y * s - kHalf * s >= 0 && y * s + kHalf * s < job.height;
    const int X = x * s, Y = y * s;
    const int d_hi = min(rule.d_cap, X - kHalf * s), range = d_hi - rule.d_lo + 1;
    const int sw = range - 1 + 2 * kHalf * s + 1;  // strip columns X - d_hi - 4 s .. X - d_lo + 4 s, all inside the image
    if (inside && range >= 3 && range <= kMaxRange && sw <= sw_max) {
      const int x0 = X - d_hi - kHalf * s;
      for (int j = 0; j < kSide; j++) {
        const uint8_t *row = job.right + static_cast<long long>(Y + (j - kHalf) * s) * job.rstride + x0;
        for (int k = lane; k < sw; k += 64) strip[j * sw + k] = row[k];
      }
      for (int k = lane; k < kSide * kSide; k += 64) {
        const int i = k % kSide, j = k / kSide;
        left[k] = job.left[static_cast<long long>(Y + (j - kHalf) * s) * job.lstride + X + (i - kHalf) * s];
      }
      wave_sync();
      // keys of the five windows: full, sample columns 0-4, 4-8, rows 0-4, 4-8
      uint32_t key[5] = {kNoKey, kNoKey, kNoKey, kNoKey, kNoKey};
      for (int base = 0; base < range; base += 64) {
        const int idx = base + lane;
        const bool live = idx < range;
        const int col0 = range - 1 - (live ? idx : range - 1);  // column of sample i = 0 in the strip: (X - d - 4 s) - x0 = d_hi - d
        uint32_t g[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // [rows < 4, = 4, > 4][columns alike]
        // the rows are walked, not unrolled: nine offsets i s in registers instead of 81 of j sw + i s
        const uint8_t *l = left, *r = strip + col0;
#pragma nounroll
        for (int j = 0; j < kHalf; j++, l += kSide, r += sw) row_sad(l, r, s, g[0]);
        row_sad(l, r, s, g[1]);
        l += kSide;
        r += sw;
#pragma nounroll
        for (int j = 0; j < kHalf; j++, l += kSide, r += sw) row_sad(l, r, s, g[2]);
        const uint32_t colL = g[0][0] + g[1][0] + g[2][0], colM = g[0][1] + g[1][1] + g[2][1], colR = g[0][2] + g[1][2] + g[2][2];
        const uint32_t rowT = g[0][0] + g[0][1] + g[0][2], rowM = g[1][0] + g[1][1] + g[1][2], rowB = g[2][0] + g[2][1] + g[2][2];
        const uint32_t S[5] = {colL + colM + colR, colL + colM, colM + colR, rowT + rowM, rowM + rowB};
        if (live) {
          cost[idx] = S[0];
#pragma unroll
          for (int k = 0; k < 5; k++) key[k] = min(key[k], S[k] * kMaxRange + static_cast<uint32_t>(idx));
        }
      }
      uint32_t best[5];
#pragma unroll
      for (int k = 0; k < 5; k++) best[k] = wave_min_u32(key[k]);
      wave_sync();
      const int i0 = static_cast<int>(best[0] % kMaxRange), S0 = static_cast<int>(best[0] / kMaxRange);
      uint32_t s2 = kNoKey;
      for (int idx = lane; idx < range; idx += 64)
        if (idx < i0 - 1 || idx > i0 + 1) s2 = min(s2, cost[idx]);
      s2 = wave_min_u32(s2);
      bool edge = false;
#pragma unroll
      for (int k = 1; k < 5; k++) {
        const int ik = static_cast<int>(best[k] % kMaxRange);
        edge = edge || ik < i0 - 1 || ik > i0 + 1;
      }
      if (S0 > rule.max_cost || i0 == 0 || i0 == range - 1) {
        status = SDVL_STEREO_NOMATCH;
      } else if (s2 != kNoKey && 100ull * static_cast<unsigned long long>(S0) > static_cast<unsigned long long>(rule.uniqueness) * s2) {
        status = SDVL_STEREO_AMBIGUOUS;
      } else if (edge) {
        status = SDVL_STEREO_EDGE;
      } else {
        status = SDVL_STEREO_OK;
        if (lane == 0) {
          const int sm = static_cast<int>(cost[i0 - 1]), sp = static_cast<int>(cost[i0 + 1]);
          const int den = sm - 2 * S0 + sp;
          const double delta = den > 0 ? 0.5 * static_cast<double>(sm - sp) / static_cast<double>(den) : 0.0;
          disparity = static_cast<double>(rule.d_lo + i0) + delta;
          z = rule.fb / disparity;
        }
      }
    }
  }
  if (lane == 0) {
    out_z[c] = z;
    out_disparity[c] = disparity;
    out_status[c] = static_cast<uint8_t>(status);
  }
}

// floor(q) as an int, cut at 512 (beyond every disparity) and at 0; NaN -> 0
int floor_cut(double q) {
  if (!(q > 0.0)) return 0;
  return q >= static_cast<double>(kMaxRange) ? kMaxRange : static_cast<int>(floor(q));
}

}  // namespace

extern "C" int sdvl_stereo_depth(sdvl_ctx *ctx, int n_jobs, const sdvl_stereo_job *jobs, int n_corners, const int32_t *xyl, const sdvl_camera *cam,
                                 const sdvl_stereo_params *p, double *out_z, double *out_disparity, uint8_t *out_status, int32_t *out_ok_per_job) {
  if (!ctx) return SDVL_ERR_INVALID;
  SDVL_REQUIRE(ctx, n_jobs >= 0 && n_corners >= 0, "sdvl_stereo_depth: negative count");
  SDVL_REQUIRE(ctx, p != nullptr, "sdvl_stereo_depth: null parameters (the baseline has no default)");
  SDVL_REQUIRE(ctx, p->baseline > 0.0 && p->baseline <= 1.79769313486231570815e308, "sdvl_stereo_depth: baseline is not a positive finite number");
  SDVL_REQUIRE(ctx, p->min_depth >= 0.0 && p->min_depth <= 1.79769313486231570815e308 && p->max_depth >= 0.0 && p->max_depth <= 1.79769313486231570815e308,
               "sdvl_stereo_depth: min_depth / max_depth negative or not finite");
  SDVL_REQUIRE(ctx, p->max_disparity >= 0 && p->max_disparity <= SDVL_STEREO_MAX_DISPARITY, "sdvl_stereo_depth: max_disparity outside 1 .. 511");
  SDVL_REQUIRE(ctx, p->uniqueness >= 0 && p->uniqueness <= 100, "sdvl_stereo_depth: uniqueness outside 1 .. 100");
  SDVL_REQUIRE(ctx, p->max_sad >= 0 && p->max_sad <= 255, "sdvl_stereo_depth: max_sad outside 1 .. 255");
  SDVL_REQUIRE(ctx, !(p->dist && p->dist->d[0] != 0.0), "sdvl_stereo_depth: a lens (dist->d[0] != 0): rectified pairs only");
  if (n_jobs == 0 || n_corners == 0) {
    for (int j = 0; j < n_jobs && out_ok_per_job; j++) out_ok_per_job[j] = 0;
    return SDVL_OK;
  }
  SDVL_REQUIRE(ctx, jobs && xyl && cam && out_z && out_disparity && out_status && out_ok_per_job, "sdvl_stereo_depth: null pointer");
  SDVL_REQUIRE(ctx, cam->fx > 0.0 && cam->fx <= 1.79769313486231570815e308, "sdvl_stereo_depth: fx is not a positive finite number");
  // the rule with its defaults (0.3 m, no upper limit, 192, 20 per sample, 80)
  const double min_depth = p->min_depth != 0.0 ? p->min_depth : 0.3;
  StereoRule rule;
  rule.fb = cam->fx * p->baseline;
  rule.d_lo = p->max_depth > 0.0 ? floor_cut(rule.fb / p->max_depth) : 0;
  rule.d_cap = floor_cut(rule.fb / min_depth);
  const int max_disparity = p->max_disparity ? p->max_disparity : 192;
  rule.d_cap = rule.d_cap < max_disparity ? rule.d_cap : max_disparity;
  rule.max_cost = kSide * kSide * (p->max_sad ? p->max_sad : 20);
  rule.uniqueness = p->uniqueness ? p->uniqueness : 80;
  // staging: jobs | corners | the job of every corner (-1: none); d_out and h_out: z | disparity | status
  sdvl_layout st, o;
  const sdvl_part<StereoJobDev> st_jobs = st.take<StereoJobDev>(n_jobs);
  const sdvl_part<int32_t> st_xyl = st.take<int32_t>(3 * static_cast<size_t>(n_corners)), st_cj = st.take<int32_t>(n_corners);
  const sdvl_part<double> o_z = o.take<double>(n_corners), o_disp = o.take<double>(n_corners);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n_corners);
  void *hs = nullptr, *ds = nullptr;
  int rc = sdvl_reserve_out_stage(ctx, o.bytes(), st.bytes(), &hs, &ds);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_stereo_job &jb = jobs[j];
    SDVL_REQUIRE(ctx, jb.left != nullptr && jb.right != nullptr, "sdvl_stereo_depth: null image");
    SDVL_REQUIRE(ctx, jb.left->home == ctx, "sdvl_stereo_depth: the left frame belongs to another context");
    SDVL_REQUIRE(ctx, jb.stride >= jb.left->width, "sdvl_stereo_depth: stride smaller than the width");
    SDVL_REQUIRE(ctx, jb.c_begin >= 0 && jb.c_begin <= jb.c_end && jb.c_end <= n_corners, "sdvl_stereo_depth: corner range outside the corner list");
  }
  SDVL_REQUIRE(ctx, !sdvl_item_jobs_fill(n_corners, n_jobs, jobs, st_cj.in(hs)), "sdvl_stereo_depth: corner ranges overlap");
  int max_level = 0;
  for (int j = 0; j < n_jobs; j++)
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++) {
      const int l = xyl[3 * i + 2];
      SDVL_REQUIRE(ctx, l >= 0 && l < jobs[j].left->v.levels, "sdvl_stereo_depth: a corner's level lies outside the left frame's pyramid");
      max_level = l > max_level ? l : max_level;
    }
  // a right image in HBM is read where it lies; one in host memory is copied to HBM first (a keyframe's corners read its rows many times
  // over), through the buffers the context keeps for depth images
  rc = sdvl_depth_pool_scope(ctx);
  if (rc) return rc;
  StereoJobDev *hj = st_jobs.in(hs);
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_stereo_job &jb = jobs[j];
    const sdvl_frame *f = jb.left;
    hj[j] = StereoJobDev{f->v.level[0], static_cast<const uint8_t *>(jb.right), f->v.lw[0], jb.stride, f->width, f->height};
    if (jb.on_device) continue;
    const uint8_t *staged = nullptr;
    rc = sdvl_depth_stage_image(ctx, jb.right, jb.stride, SDVL_DEPTH_RIGHT8, f->width, f->height, static_cast<size_t>(f->width), &staged);
    if (rc) return rc;
    hj[j].right = staged;
    hj[j].rstride = f->width;
  }
  memcpy(st_xyl.in(hs), xyl, st_xyl.bytes());
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  const int sw_max = (rule.d_cap - rule.d_lo) + 2 * kHalf * (1 << max_level) + 1;  // (a call whose range is empty launches all the same: OUTSIDE)
  const size_t lds_bytes = kMaxRange * sizeof(uint32_t) + kLeftBytes + static_cast<size_t>(kSide) * (sw_max > 1 ? sw_max : 1);
  SDVL_REQUIRE(ctx, lds_bytes <= 64 * 1024, "sdvl_stereo_depth: the right strip does not fit the LDS");
  SDVL_LAUNCH_LDS(ctx, "stereo_depth", stereo_depth, dim3(n_corners), dim3(64), lds_bytes, st_jobs.cin(ds), st_xyl.cin(ds), st_cj.cin(ds), rule, sw_max,
                  o_z.in(ctx->d_out), o_disp.in(ctx->d_out), o_status.in(ctx->d_out));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  rc = sdvl_collect_out(ctx, o.bytes());
  if (rc) return rc;
  memcpy(out_z, o_z.in(ctx->h_out), o_z.bytes());
  memcpy(out_disparity, o_disp.in(ctx->h_out), o_disp.bytes());
  memcpy(out_status, o_status.in(ctx->h_out), o_status.bytes());
  sdvl_ok_per_job(n_jobs, jobs, out_status, SDVL_STEREO_OK, out_ok_per_job);
  return SDVL_OK;
}
