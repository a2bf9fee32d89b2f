// sdvl_stereo.hip — stereo cameras: the depth of a keyframe's filtered corners from a rectified right image (sdvl_stereo_depth), the
// producer of the `z` / `status` contract that sdvl_depth_seed fills for a depth camera; and the same matcher at positions of the caller's
// own (sdvl_stereo_lookup: the sub-pixel position a feature was found at, the stride of the level it was found on), which is to
// sdvl_stereo_depth what sdvl_depth_lookup is to sdvl_depth_seed.  A sparse matcher: costs are taken at the corners only, never a dense
// disparity image.  The rule is this project's own; tests/stereo_restatement.py and tests/stereo_lookup_restatement.py are its specification:
//   centre    a corner (x, y, l): (X, Y) = (x << l, y << l); a position (px, py) found on level l: (X, Y) = (floor(px + 0.5), floor(py + 0.5)),
//             which need not be a multiple of s; s = 1 << l in both
//   window    the 9 x 9 samples at (X + i s, Y + j s), i, j in -4 .. 4, of level 0 of both images
//   range     d_lo = floor(fx b / max_depth) (no max_depth: 0), d_hi = min(max_disparity, floor(fx b / min_depth), X - 4 s)
//   cost      S(d) = sum |L - R| over the 81 samples, an integer <= 20 655; d0 its argmin, ties to the smallest d; four half-window costs
//             from the same absolute differences (sample columns 0-4, 4-8, rows 0-4, 4-8)
//   status    the first that applies of OUTSIDE (left window off the image, fewer than 3 disparities), NOMATCH (S(d0) > 81 max_sad, d0 an
//             end of the range), AMBIGUOUS (100 S(d0) > uniqueness S2, S2 = min S(d) over |d - d0| > 1), EDGE (a half window's argmin
//             differs from d0 by more than 1); otherwise OK
//   result    delta = 0.5 (S- - S+) / (S- - 2 S0 + S+) (denominator > 0, else 0), disparity = d0 + delta, z = fx b / disparity
// stereo_depth, stereo_lookup: one wave per corner / position, lane per disparity (d_lo + lane + 64 k, at most 8 rounds).  Both call
// stereo_match, the one statement of the rule at (X, Y, s): the wave stages the right strip — 9 rows x (range + 8 s) bytes — and the 81
// left samples in LDS; a lane sums its 81 absolute differences into nine accumulators (sample columns < 4, = 4, > 4 times rows alike),
// from which the full and the four half-window costs are sums.  The five argmins are 32-bit minima over keys S 512 + index
// (wave_min_u32: DPP steps); the costs go to LDS, from which S2, S- and S+ are read.  No floating point before the parabola, which one
// lane evaluates in double, in the restatement's operation order (-ffp-contract=off).
#include <string>

#include "sdvl_stereo_device.h"
#include "sdvl_wave.h"

using namespace sdvl_stereo;

namespace {

constexpr int kHalf = 4, kSide = 2 * kHalf + 1;   // the window
constexpr int kMaxRange = 512;                    // disparities 0 .. 511: 8 rounds of 64 lanes
constexpr int kLeftBytes = 96;                    // 81 left samples, padded
constexpr uint32_t kNoKey = 0xffffffffu;
constexpr int kNoLookup = 255;                    // the status of a request whose wave looked nothing up

// one row of a window: the nine absolute differences into the sums of sample columns < 4, = 4, > 4
__device__ __forceinline__ void row_sad(const uint8_t *l, const uint8_t *r, int s, uint32_t g[3]) {
#pragma unroll
  for (int i = 0; i < kSide; i++) {
    const int a = l[i], b = r[i * s];
    g[i < kHalf ? 0 : i == kHalf ? 1 : 2] += static_cast<uint32_t>(a > b ? a - b : b - a);
  }
}

// what a wave leaves of one centre; disparity and z hold the result in lane 0 alone
struct StereoMatch {
  int status;
  double disparity, z;
};

// The rule at the level-0 centre (X, Y) with the stride s, by one whole wave (every argument the same in all lanes, so the wave leaves
// the branches together).  0 <= X, Y < 16384 and s <= 128: nothing below overflows.  lds: the block's dynamic LDS,
// cost[512] uint32 | left[96] | strip[9][rule.sw_max]
__device__ __forceinline__ StereoMatch stereo_match(const StereoJobDev &job, int X, int Y, int s, const StereoRule &rule, uint32_t *lds) {
  uint32_t *cost = lds;
  uint8_t *left = reinterpret_cast<uint8_t *>(lds + kMaxRange);
  uint8_t *strip = left + kLeftBytes;
  const int lane = threadIdx.x;
  StereoMatch m = {SDVL_STEREO_OUTSIDE, 0.0, 0.0};
  const bool inside = X - kHalf * s >= 0 && X + kHalf * s < job.width && Y - kHalf * s >= 0 && Y + kHalf * s < job.height;
  const int d_hi = min(rule.d_cap, X - kHalf * s), range = d_hi - rule.d_lo + 1;
  const int sw = range - 1 + 2 * kHalf * s + 1;  // strip columns X - d_hi - 4 s .. X - d_lo + 4 s, all inside the image
  if (!(inside && range >= 3 && range <= kMaxRange && sw <= rule.sw_max)) return m;
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
    m.status = SDVL_STEREO_NOMATCH;
  } else if (s2 != kNoKey && 100ull * static_cast<unsigned long long>(S0) > static_cast<unsigned long long>(rule.uniqueness) * s2) {
    m.status = SDVL_STEREO_AMBIGUOUS;
  } else if (edge) {
    m.status = SDVL_STEREO_EDGE;
  } else {
    m.status = SDVL_STEREO_OK;
    if (lane == 0) {
      const int sm = static_cast<int>(cost[i0 - 1]), sp = static_cast<int>(cost[i0 + 1]);
      const int den = sm - 2 * S0 + sp;
      const double delta = den > 0 ? 0.5 * static_cast<double>(sm - sp) / static_cast<double>(den) : 0.0;
      m.disparity = static_cast<double>(rule.d_lo + i0) + delta;
      m.z = rule.fb / m.disparity;
    }
  }
  return m;
}

// Dynamic LDS of the block (one wave): stereo_match's
__global__ __launch_bounds__(64) void stereo_depth(const StereoJobDev *__restrict__ jobs, const int32_t *__restrict__ xyl,
                                                   const int32_t *__restrict__ corner_job, StereoRule rule, double *__restrict__ out_z,
                                                   double *__restrict__ out_disparity, uint8_t *__restrict__ out_status) {
  extern __shared__ uint32_t lds[];
  const int c = blockIdx.x;
  const int jb = corner_job[c];
  StereoMatch m = {SDVL_STEREO_NOMATCH, 0.0, 0.0};  // a corner no job names
  if (jb >= 0) {
    const StereoJobDev job = jobs[jb];
    const int x = xyl[3 * c], y = xyl[3 * c + 1], s = 1 << xyl[3 * c + 2];
    m.status = SDVL_STEREO_OUTSIDE;
    // (x, y < 16384 before they are scaled: no overflow)
    if (x >= 0 && y >= 0 && x < job.width && y < job.height) m = stereo_match(job, x * s, y * s, s, rule, lds);
  }
  if (threadIdx.x == 0) {
    out_z[c] = m.z;
    out_disparity[c] = m.disparity;
    out_status[c] = static_cast<uint8_t>(m.status);
  }
}

// The same at a position of its own: one wave per position.  kSearch false: px2, level and pos_job as sdvl_stereo_lookup's caller states
// them (levels checked on the host); a position no job names is NOMATCH.  kSearch true: the results a search left in HBM — the wave of
// a miss or of a request in no job writes status 255 and leaves at once; the level is clamped as the measured depth filter clamps it.
// out_disparity may be null
template <bool kSearch>
__device__ __forceinline__ void stereo_lookup_wave(const StereoJobDev *__restrict__ jobs, const double *__restrict__ px2,
                                                   const int32_t *__restrict__ level, const sdvl_search_res *__restrict__ res,
                                                   const int32_t *__restrict__ pos_job, const StereoRule &rule, uint32_t *lds,
                                                   double *__restrict__ out_z, double *__restrict__ out_disparity,
                                                   uint8_t *__restrict__ out_status) {
  const int c = blockIdx.x;
  const int jb = pos_job[c];
  StereoMatch m = {kSearch ? kNoLookup : SDVL_STEREO_NOMATCH, 0.0, 0.0};
  bool named = jb >= 0;
  double px = 0.0, py = 0.0;
  int l = 0;
  if constexpr (kSearch) {
    named = named && res[c].found != 0;
    if (named) {
      px = res[c].px[0], py = res[c].px[1];
      l = res[c].level < 0 ? 0 : (res[c].level >= SDVL_MAX_LEVELS ? SDVL_MAX_LEVELS - 1 : res[c].level);
    }
  } else if (named) {
    px = px2[2 * c], py = px2[2 * c + 1];
    l = level[c];
  }
  if (named) {
    const StereoJobDev job = jobs[jb];
    const double fu = floor(px + 0.5), fv = floor(py + 0.5);
    m.status = SDVL_STEREO_OUTSIDE;
    // (a NaN centre fails the comparisons: OUTSIDE; one inside the image converts exactly)
    if (fu >= 0.0 && fu < job.width && fv >= 0.0 && fv < job.height) m = stereo_match(job, static_cast<int>(fu), static_cast<int>(fv), 1 << l, rule, lds);
  }
  if (threadIdx.x == 0) {
    out_z[c] = m.z;
    if (out_disparity) out_disparity[c] = m.disparity;
    out_status[c] = static_cast<uint8_t>(m.status);
  }
}

__global__ __launch_bounds__(64) void stereo_lookup(const StereoJobDev *__restrict__ jobs, const double *__restrict__ px2,
                                                    const int32_t *__restrict__ level, const int32_t *__restrict__ pos_job, StereoRule rule,
                                                    double *__restrict__ out_z, double *__restrict__ out_disparity,
                                                    uint8_t *__restrict__ out_status) {
  extern __shared__ uint32_t lds[];
  stereo_lookup_wave<false>(jobs, px2, level, nullptr, pos_job, rule, lds, out_z, out_disparity, out_status);
}

__global__ __launch_bounds__(64) void stereo_lookup_found(const StereoJobDev *__restrict__ jobs, const sdvl_search_res *__restrict__ res,
                                                          const int32_t *__restrict__ req_job, StereoRule rule, double *__restrict__ out_z,
                                                          uint8_t *__restrict__ out_status) {
  extern __shared__ uint32_t lds[];
  stereo_lookup_wave<true>(jobs, nullptr, nullptr, res, req_job, rule, lds, out_z, nullptr, out_status);
}

// floor(q) as an int, cut at 512 (beyond every disparity) and at 0; NaN -> 0
int floor_cut(double q) {
  if (!(q > 0.0)) return 0;
  return q >= static_cast<double>(kMaxRange) ? kMaxRange : static_cast<int>(floor(q));
}

// ---- sdvl_stereo_depth and sdvl_stereo_lookup: one body (stereo_items_run) over what each states of its own — its inputs, their parts
// of the staging block and how they are filled, the level of an item, and its launch
struct CornerStage {  // staging: jobs | corners | the job of every corner (-1: none)
  static constexpr const char *who = "sdvl_stereo_depth", *item = "corner";
  const int32_t *xyl;
  sdvl_part<int32_t> st_xyl;
  bool stated() const { return xyl != nullptr; }
  int level(int i) const { return xyl[3 * i + 2]; }
  void take(sdvl_layout &st, int n) { st_xyl = st.take<int32_t>(3 * static_cast<size_t>(n)); }
  void fill(void *hs) const { memcpy(st_xyl.in(hs), xyl, st_xyl.bytes()); }
  template <typename... Tail>
  void launch(sdvl_ctx *ctx, const void *ds, int n, size_t lds_bytes, const StereoJobDev *jobs, const int32_t *item_job, Tail... tail) const {
    SDVL_LAUNCH_LDS(ctx, "stereo_depth", stereo_depth, dim3(n), dim3(64), lds_bytes, jobs, st_xyl.cin(ds), item_job, tail...);
  }
};

struct PositionStage {  // staging: jobs | positions | levels | the job of every position (-1: none)
  static constexpr const char *who = "sdvl_stereo_lookup", *item = "position";
  const double *px2;
  const int32_t *lv;
  sdvl_part<double> st_px;
  sdvl_part<int32_t> st_level;
  bool stated() const { return px2 != nullptr && lv != nullptr; }
  int level(int i) const { return lv[i]; }
  void take(sdvl_layout &st, int n) { st_px = st.take<double>(2 * static_cast<size_t>(n)), st_level = st.take<int32_t>(n); }
  void fill(void *hs) const { memcpy(st_px.in(hs), px2, st_px.bytes()), memcpy(st_level.in(hs), lv, st_level.bytes()); }
  template <typename... Tail>
  void launch(sdvl_ctx *ctx, const void *ds, int n, size_t lds_bytes, const StereoJobDev *jobs, const int32_t *item_job, Tail... tail) const {
    SDVL_LAUNCH_LDS(ctx, "stereo_lookup", stereo_lookup, dim3(n), dim3(64), lds_bytes, jobs, st_px.cin(ds), st_level.cin(ds), item_job, tail...);
  }
};

// d_out and h_out: z | disparity | status
template <typename Stage>
int stereo_items_run(sdvl_ctx *ctx, Stage &stage, int n_jobs, const sdvl_stereo_job *jobs, int n, const sdvl_camera *cam, const sdvl_stereo_params *p,
                     double *out_z, double *out_disparity, uint8_t *out_status, int32_t *out_ok_per_job) {
  if (!ctx) return SDVL_ERR_INVALID;
  const std::string w(Stage::who), item(Stage::item);
  SDVL_REQUIRE(ctx, n_jobs >= 0 && n >= 0, w + ": negative count");
  StereoRule rule;
  int rc = sdvl_stereo_rule_of(ctx, Stage::who, nullptr, p, &rule);
  if (rc) return rc;
  if (n_jobs == 0 || n == 0) {
    for (int j = 0; j < n_jobs && out_ok_per_job; j++) out_ok_per_job[j] = 0;
    return SDVL_OK;
  }
  SDVL_REQUIRE(ctx, jobs && stage.stated() && cam && out_z && out_disparity && out_status && out_ok_per_job, w + ": null pointer");
  rc = sdvl_stereo_rule_of(ctx, Stage::who, cam, p, &rule);
  if (rc) return rc;
  sdvl_layout st, o;
  const sdvl_part<StereoJobDev> st_jobs = st.take<StereoJobDev>(n_jobs);
  stage.take(st, n);
  const sdvl_part<int32_t> st_item_job = st.take<int32_t>(n);
  const sdvl_part<double> o_z = o.take<double>(n), o_disp = o.take<double>(n);
  const sdvl_part<uint8_t> o_status = o.take<uint8_t>(n);
  void *hs = nullptr, *ds = nullptr;
  rc = sdvl_reserve_out_stage(ctx, o.bytes(), st.bytes(), &hs, &ds);
  if (!rc) rc = sdvl_stereo_jobs_check(ctx, Stage::who, Stage::item, n_jobs, jobs, n);
  if (rc) return rc;
  SDVL_REQUIRE(ctx, !sdvl_item_jobs_fill(n, n_jobs, jobs, st_item_job.in(hs)), w + ": " + item + " ranges overlap");
  int max_level = 0;
  for (int j = 0; j < n_jobs; j++)
    for (int i = jobs[j].c_begin; i < jobs[j].c_end; i++) {
      const int l = stage.level(i);
      SDVL_REQUIRE(ctx, l >= 0 && l < jobs[j].left->v.levels, w + ": a " + item + "'s level lies outside the left frame's pyramid");
      max_level = l > max_level ? l : max_level;
    }
  size_t lds_bytes = 0;
  rc = sdvl_stereo_lds(ctx, Stage::who, max_level, &rule, &lds_bytes);
  if (!rc) rc = sdvl_stereo_jobs_resolve(ctx, n_jobs, jobs, st_jobs.in(hs));
  if (rc) return rc;
  stage.fill(hs);
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, ds, hs, st.bytes()));
  stage.launch(ctx, ds, n, lds_bytes, st_jobs.cin(ds), st_item_job.cin(ds), rule, o_z.in(ctx->d_out), o_disp.in(ctx->d_out), o_status.in(ctx->d_out));
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  rc = sdvl_collect_out(ctx, o.bytes());
  if (rc) return rc;
  memcpy(out_z, o_z.in(ctx->h_out), o_z.bytes());
  memcpy(out_disparity, o_disp.in(ctx->h_out), o_disp.bytes());
  memcpy(out_status, o_status.in(ctx->h_out), o_status.bytes());
  sdvl_ok_per_job(n_jobs, jobs, out_status, SDVL_STEREO_OK, out_ok_per_job);
  return SDVL_OK;
}

}  // namespace

// ---- what the entries that take stereo jobs share (sdvl_stereo_device.h)
// cam null: the parameters' refusals alone (what an entry checks before it knows that there is work)
int sdvl_stereo_rule_of(sdvl_ctx *ctx, const char *who, const sdvl_camera *cam, const sdvl_stereo_params *p, StereoRule *rule) {
  const std::string w(who);
  const double big = 1.79769313486231570815e308;
  SDVL_REQUIRE(ctx, p != nullptr, w + ": null parameters (the baseline has no default)");
  SDVL_REQUIRE(ctx, p->baseline > 0.0 && p->baseline <= big, w + ": baseline is not a positive finite number");
  SDVL_REQUIRE(ctx, p->min_depth >= 0.0 && p->min_depth <= big && p->max_depth >= 0.0 && p->max_depth <= big,
               w + ": min_depth / max_depth negative or not finite");
  SDVL_REQUIRE(ctx, p->max_disparity >= 0 && p->max_disparity <= SDVL_STEREO_MAX_DISPARITY, w + ": max_disparity outside 1 .. 511");
  SDVL_REQUIRE(ctx, p->uniqueness >= 0 && p->uniqueness <= 100, w + ": uniqueness outside 1 .. 100");
  SDVL_REQUIRE(ctx, p->max_sad >= 0 && p->max_sad <= 255, w + ": max_sad outside 1 .. 255");
  SDVL_REQUIRE(ctx, !(p->dist && p->dist->d[0] != 0.0), w + ": a lens (dist->d[0] != 0): rectified pairs only");
  if (!cam) return SDVL_OK;
  SDVL_REQUIRE(ctx, cam->fx > 0.0 && cam->fx <= big, w + ": fx is not a positive finite number");
  // the rule with its defaults (0.3 m, no upper limit, 192, 20 per sample, 80)
  const double min_depth = p->min_depth != 0.0 ? p->min_depth : 0.3;
  rule->fb = cam->fx * p->baseline;
  rule->d_lo = p->max_depth > 0.0 ? floor_cut(rule->fb / p->max_depth) : 0;
  rule->d_cap = floor_cut(rule->fb / min_depth);
  const int max_disparity = p->max_disparity ? p->max_disparity : 192;
  rule->d_cap = rule->d_cap < max_disparity ? rule->d_cap : max_disparity;
  rule->max_cost = kSide * kSide * (p->max_sad ? p->max_sad : 20);
  rule->uniqueness = p->uniqueness ? p->uniqueness : 80;
  rule->sw_max = 0;
  rule->pad_ = 0;
  return SDVL_OK;
}

int sdvl_stereo_jobs_check(sdvl_ctx *ctx, const char *who, const char *item, int n_jobs, const sdvl_stereo_job *jobs, int n) {
  const std::string w(who);
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_stereo_job &jb = jobs[j];
    SDVL_REQUIRE(ctx, jb.left != nullptr && jb.right != nullptr, w + ": null image");
    SDVL_REQUIRE(ctx, jb.left->home == ctx, w + ": the left frame belongs to another context");
    SDVL_REQUIRE(ctx, jb.stride >= jb.left->width, w + ": stride smaller than the width");
    SDVL_REQUIRE(ctx, jb.c_begin >= 0 && jb.c_begin <= jb.c_end && jb.c_end <= n, w + ": " + item + " range outside the " + item + " list");
  }
  return SDVL_OK;
}

// a right image in HBM is read where it lies; one in host memory is copied to HBM first (a keyframe's corners read its rows many times
// over), through the buffers the context keeps for depth images
int sdvl_stereo_jobs_resolve(sdvl_ctx *ctx, int n_jobs, const sdvl_stereo_job *jobs, StereoJobDev *out) {
  int rc = sdvl_depth_pool_scope(ctx);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; j++) {
    const sdvl_stereo_job &jb = jobs[j];
    const sdvl_frame *f = jb.left;
    out[j] = StereoJobDev{f->v.level[0], static_cast<const uint8_t *>(jb.right), f->v.lw[0], jb.stride, f->width, f->height};
    if (jb.on_device) continue;
    const uint8_t *staged = nullptr;
    rc = sdvl_depth_stage_image(ctx, jb.right, jb.stride, SDVL_DEPTH_RIGHT8, f->width, f->height, static_cast<size_t>(f->width), &staged);
    if (rc) return rc;
    out[j].right = staged;
    out[j].rstride = f->width;
  }
  return SDVL_OK;
}

int sdvl_stereo_lds(sdvl_ctx *ctx, const char *who, int max_level, StereoRule *rule, size_t *lds_bytes) {
  const int sw_max = (rule->d_cap - rule->d_lo) + 2 * kHalf * (1 << max_level) + 1;  // (a call whose range is empty launches all the same: OUTSIDE)
  rule->sw_max = sw_max;
  *lds_bytes = kMaxRange * sizeof(uint32_t) + kLeftBytes + static_cast<size_t>(kSide) * (sw_max > 1 ? sw_max : 1);
  SDVL_REQUIRE(ctx, *lds_bytes <= 64 * 1024, std::string(who) + ": the right strip does not fit the LDS");
  return SDVL_OK;
}

int sdvl_stereo_lookup_enqueue(sdvl_ctx *ctx, int n, const StereoJobDev *d_jobs, const sdvl_search_res *d_res, const int32_t *d_req_job,
                               const StereoRule &rule, size_t lds_bytes, double *d_z, uint8_t *d_status) {
  SDVL_LAUNCH_LDS(ctx, "stereo_lookup", stereo_lookup_found, dim3(n), dim3(64), lds_bytes, d_jobs, d_res, d_req_job, rule, d_z, d_status);
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  return SDVL_OK;
}

extern "C" int sdvl_stereo_depth(sdvl_ctx *ctx, int n_jobs, const sdvl_stereo_job *jobs, int n_corners, const int32_t *xyl, const sdvl_camera *cam,
                                 const sdvl_stereo_params *p, double *out_z, double *out_disparity, uint8_t *out_status, int32_t *out_ok_per_job) {
  CornerStage stage{xyl, {}};
  return stereo_items_run(ctx, stage, n_jobs, jobs, n_corners, cam, p, out_z, out_disparity, out_status, out_ok_per_job);
}

extern "C" int sdvl_stereo_lookup(sdvl_ctx *ctx, int n_jobs, const sdvl_stereo_job *jobs, int n, const double *px2, const int32_t *level,
                                  const sdvl_camera *cam, const sdvl_stereo_params *p, double *out_z, double *out_disparity, uint8_t *out_status,
                                  int32_t *out_ok_per_job) {
  PositionStage stage{px2, level, {}, {}};
  return stereo_items_run(ctx, stage, n_jobs, jobs, n, cam, p, out_z, out_disparity, out_status, out_ok_per_job);
}
