// sdvl_bundle.hip — Bundle::Local (extra/bundle.cc:110-223) on the device: what g2o's Levenberg-Marquardt with the Schur complement
// does to a local window of keyframes and points (optimization_algorithm_levenberg.cpp:61-189, block_solver.hpp,
// base_binary_edge.hpp:60-115, robust_kernel_impl.cpp:78-91, types_six_dof_expmap.cpp:103-147).  g2o is no dependency of this project:
// tests/bundle_restatement.py states what is computed, DESIGN §2 what g2o leaves implicit.
// The kernel is a template over the depth form (sdvl_bundle_adjust_depth, tests/bundle_depth_restatement.py): an edge that carries a
// measured depth is EdgeStereoSE3ProjectXYZ (:150-234), three rows; bundle_adjust_kernel<false> is the monocular kernel as it was.
//
// One workgroup (256 threads) per problem; both stages, every iteration and every trial run inside the kernel.  Everything is FP64.
// No floating-point atomics: a point's blocks are summed by its own thread over its CSR edges, a pose's blocks by its own 16 lanes over
// the keyframe-major list (partial sums added in lane order), an entry of the reduced system by its own thread over the points in order, chi2 by a fixed tree — the same
// input gives the same bits on every run and in every batch position.
//   LDS      the reduced system (lower triangle, packed; the Cholesky factor overwrites it), its right-hand side / solution, the free
//            poses (linearisation point and trial), and a tile of per-edge blocks: 61.1 KB at the cap of 16 free poses
//   HBM      per point H_ll and b_l (9 doubles), the trial positions, R|t of every pose at the linearisation point and at the trial,
//            H_pp and its partial sums: scratch of the context.  Per-edge Jacobians are NOT kept: an edge's two Jacobians cost ~60 flops from 17 doubles that
//            sit in cache, a stored W block alone is 18 doubles per edge and trial
// Nothing in the kernel indexes by a floating-point value and every loop is bounded by the host-checked index arrays: NaN or infinite
// input ends in a status, not in a fault.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <numeric>
#include <type_traits>

#include "sdvl_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxFree = SDVL_BUNDLE_MAX_FREE;
constexpr int kMaxN = 6 * kMaxFree;                       // unknowns of the reduced system
constexpr int kPacked = kMaxN * (kMaxN + 1) / 2;
constexpr int kTile = 48;                                 // per-edge slots (and points) of one Schur tile
// entries of the reduced system's lower triangle (36 per block pair a > b, 21 per diagonal block) and of its right-hand side
constexpr int items_of(int nf) { return nf * (nf + 1) / 2 * 36 - 15 * nf + 6 * nf; }
constexpr int kItems = (items_of(kMaxFree) + kThreads - 1) / kThreads;  // per thread: 19
constexpr double kChi2Th = 5.991;       // 95 % of chi2 with two degrees of freedom: the monocular edge
constexpr double kChi2ThDepth = 7.815;  // with three: the depth edge
constexpr int kMaxTrials = 10;

struct EdgeDev {  // CSR (point-major) order
  int32_t pt, kf;  // relative to the problem
  double u, v;
};

struct ProblemDev {
  int32_t kf_begin, n_kf, n_free;
  int32_t pt_begin, n_pt;
  int32_t e_begin, n_e;
  int32_t ptoff_begin;  // of the problem's n_pt + 1 entries in pt_off and pt_fe_off
  int32_t kfoff_begin;  // of its n_kf + 1 entries in kf_off
  int32_t tile_begin, n_tiles;  // of its n_tiles + 1 entries in tile_pt
  int32_t status;       // decided on the host: SDVL_BUNDLE_EMPTY / _NO_EDGES, else 0
};

struct BundleArgs {
  const ProblemDev *problems;
  const EdgeDev *edges;
  const int32_t *pt_off;     // CSR: absolute edge range of every point
  const int32_t *kf_off;     // keyframe-major: range in kf_edges of every pose
  const int32_t *kf_edges;   // absolute edge indices, ascending per pose
  const int32_t *pt_fe_off;  // range in fe of every point
  const int32_t *fe;         // absolute indices of the edges to free poses, point-major
  const int32_t *tile_pt;    // point boundaries of the Schur tiles (relative to the problem)
  double *poses;             // [n_kf][7] in / out
  double *points;            // [n_pt][3] in / out: the linearisation point (= the accepted estimates)
  double *pts_trial;         // [n_pt][3]
  double *ptblk;             // [n_pt][9]: H_ll (00 01 02 11 12 22), b_l
  double *rt_lin, *rt_trial; // [n_kf][12]: R row-major, t
  double *hpp;               // [n_problems][kMaxFree][36]
  double *hpart;             // [n_problems][kMaxFree][16][27]: partial sums of H_pp (lower triangle) and b_p
  int32_t *levels;           // [n_e] CSR order
  int32_t *pose_stages, *point_stages;
  sdvl_bundle_result *results;
  double fx, fy, cx, cy;
};

// the depth form (sdvl_bundle_adjust_depth): EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:150-234) on the edges that carry a
// measured depth; tests/bundle_depth_restatement.py states it.  The monocular form neither reads nor holds any of this.
struct BundleArgsD : BundleArgs {
  const double *edge_depth;  // [n_e] CSR order: measured camera-frame z, <= 0: a monocular edge
  double bf;
};
template <bool kDepth>
using ArgsOf = std::conditional_t<kDepth, BundleArgsD, BundleArgs>;

struct Geo {
  double x, y, z, ex, ey;
  double ez;  // depth form only: (u - bf / d) - (u' - bf / z), 0 on an edge without a depth
};

template <bool kDepth>
__device__ __forceinline__ Geo edge_geo(const double *__restrict__ rt, const double *__restrict__ X, double u, double v, double d, const ArgsOf<kDepth> &A) {
  Geo g;
  g.x = ((rt[0] * X[0] + rt[1] * X[1]) + rt[2] * X[2]) + rt[9];
  g.y = ((rt[3] * X[0] + rt[4] * X[1]) + rt[5] * X[2]) + rt[10];
  g.z = ((rt[6] * X[0] + rt[7] * X[1]) + rt[8] * X[2]) + rt[11];
  g.ex = u - (A.fx * g.x / g.z + A.cx);
  g.ey = v - (A.fy * g.y / g.z + A.cy);
  if constexpr (kDepth) g.ez = d > 0.0 ? (u - A.bf / d) - ((A.fx * g.x / g.z + A.cx) - A.bf / g.z) : 0.0;
  return g;
}

// err.err, rows summed ((r0 + r1) + r2)
template <bool kDepth>
__device__ __forceinline__ double edge_chi2(const Geo &g) {
  double e = g.ex * g.ex + g.ey * g.ey;
  if constexpr (kDepth) e = e + g.ez * g.ez;
  return e;
}

// the edge's outlier threshold = its Huber delta^2
template <bool kDepth>
__device__ __forceinline__ double edge_threshold(double d) {
  if constexpr (kDepth) return d > 0.0 ? kChi2ThDepth : kChi2Th;
  return kChi2Th;
}

// linearizeOplus, types_six_dof_expmap.cpp:103-139; the depth form's row 2 is row 0 plus the bf terms of :210-212 and :228-233, and
// zero on an edge without a depth
template <bool kDepth>
__device__ __forceinline__ void edge_jacobians(const Geo &g, const double *__restrict__ rt, double d, const ArgsOf<kDepth> &A, double (*Ji)[3], double (*Jj)[6]) {
  const double x = g.x, y = g.y, z = g.z, z2 = z * z;
  const double t02 = -x / z * A.fx, t12 = -y / z * A.fy, s = -1.0 / z;
  for (int c = 0; c < 3; c++) {
    Ji[0][c] = s * (A.fx * rt[c] + t02 * rt[6 + c]);
    Ji[1][c] = s * (A.fy * rt[3 + c] + t12 * rt[6 + c]);
  }
  Jj[0][0] = x * y / z2 * A.fx;
  Jj[0][1] = -(1.0 + x * x / z2) * A.fx;
  Jj[0][2] = y / z * A.fx;
  Jj[0][3] = -1.0 / z * A.fx;
  Jj[0][4] = 0.0;
  Jj[0][5] = x / z2 * A.fx;
  Jj[1][0] = (1.0 + y * y / z2) * A.fy;
  Jj[1][1] = -x * y / z2 * A.fy;
  Jj[1][2] = -x / z * A.fy;
  Jj[1][3] = 0.0;
  Jj[1][4] = -1.0 / z * A.fy;
  Jj[1][5] = y / z2 * A.fy;
  if constexpr (kDepth) {
    const bool has = d > 0.0;
    for (int c = 0; c < 3; c++) Ji[2][c] = has ? Ji[0][c] - A.bf * rt[6 + c] / z2 : 0.0;
    Jj[2][0] = has ? Jj[0][0] - A.bf * y / z2 : 0.0;
    Jj[2][1] = has ? Jj[0][1] + A.bf * x / z2 : 0.0;
    Jj[2][2] = has ? Jj[0][2] : 0.0;
    Jj[2][3] = has ? Jj[0][3] : 0.0;
    Jj[2][4] = 0.0;
    Jj[2][5] = has ? Jj[0][5] - A.bf / z2 : 0.0;
  }
}

// sum over the edge's rows of A[k][i] B[k][j] and of A[k][i] err[k], ((r0 + r1) + r2)
template <bool kDepth, int NA, int NB>
__device__ __forceinline__ double rows_jj(const double (*A)[NA], int i, const double (*B)[NB], int j) {
  double s = A[0][i] * B[0][j] + A[1][i] * B[1][j];
  if constexpr (kDepth) s = s + A[2][i] * B[2][j];
  return s;
}
template <bool kDepth, int NA>
__device__ __forceinline__ double rows_je(const double (*A)[NA], int i, const Geo &g) {
  double s = A[0][i] * g.ex + A[1][i] * g.ey;
  if constexpr (kDepth) s = s + A[2][i] * g.ez;
  return s;
}

// RobustKernelHuber::robustify, robust_kernel_impl.cpp:78-91: rho[0] -> *cost, returns rho[1]
__device__ __forceinline__ double huber(double e, bool robust, bool depth_edge, double *cost) {
  const double delta = depth_edge ? sqrt(kChi2ThDepth) : sqrt(kChi2Th), dsqr = delta * delta;
  if (!robust || e <= dsqr) {
    *cost = e;
    return 1.0;
  }
  const double s = sqrt(e);
  *cost = 2.0 * s * delta - dsqr;
  return delta / s;
}

// inverse of the symmetric 3x3 (h00 h01 h02 h11 h12 h22) + lam I by the adjugate, same packing
__device__ __forceinline__ void inv3_sym(const double *__restrict__ h, double lam, double *__restrict__ o) {
  const double a = h[0] + lam, b = h[1], c = h[2], d = h[3] + lam, e = h[4], f = h[5] + lam;
  const double Aa = d * f - e * e, Bb = c * e - b * f, Cc = b * e - c * d;
  const double inv = 1.0 / ((a * Aa + b * Bb) + c * Cc);
  o[0] = Aa * inv;
  o[1] = Bb * inv;
  o[2] = Cc * inv;
  o[3] = (a * f - c * c) * inv;
  o[4] = (b * c - a * e) * inv;
  o[5] = (a * d - b * b) * inv;
}

__device__ __forceinline__ void quat_to_rt(const double *__restrict__ p, double *__restrict__ rt) {
  const double w = p[0], x = p[1], y = p[2], z = p[3];
  rt[0] = 1.0 - 2.0 * (y * y + z * z); rt[1] = 2.0 * (x * y - w * z); rt[2] = 2.0 * (x * z + w * y);
  rt[3] = 2.0 * (x * y + w * z); rt[4] = 1.0 - 2.0 * (x * x + z * z); rt[5] = 2.0 * (y * z - w * x);
  rt[6] = 2.0 * (x * z - w * y); rt[7] = 2.0 * (y * z + w * x); rt[8] = 1.0 - 2.0 * (x * x + y * y);
  rt[9] = p[4]; rt[10] = p[5]; rt[11] = p[6];
}

// exp(d) * pose, d = (omega, upsilon): VertexSE3Expmap::oplusImpl, se3quat.h:223-257
__device__ void exp_update(const double *__restrict__ pose, const double *__restrict__ d, double *__restrict__ out) {
  const double ox = d[0], oy = d[1], oz = d[2];
  const double th2 = (ox * ox + oy * oy) + oz * oz, th = sqrt(th2);
  double a, b, c, qw, s;
  if (th < 1e-5) {
    a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; c = 1.0 / 6.0 - th2 / 120.0;
    qw = 1.0 - th2 / 8.0; s = 0.5 - th2 / 48.0;
  } else {  // NaN lands here: everything below is NaN, chi2 of the trial is NaN, the trial is rejected
    a = sin(th) / th; b = (1.0 - cos(th)) / th2; c = (th - sin(th)) / (th2 * th);
    qw = cos(0.5 * th); s = sin(0.5 * th) / th;
  }
  // W = skew(omega), W2 = W W
  const double W[3][3] = {{0.0, -oz, oy}, {oz, 0.0, -ox}, {-oy, ox, 0.0}};
  double W2[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) W2[i][j] = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
  double t[3];
  for (int i = 0; i < 3; i++) {
    double rt = 0.0, vu = 0.0;
    for (int j = 0; j < 3; j++) {
      const double id = i == j ? 1.0 : 0.0;
      rt += ((id + a * W[i][j]) + b * W2[i][j]) * pose[4 + j];
      vu += ((id + b * W[i][j]) + c * W2[i][j]) * d[3 + j];
    }
    t[i] = rt + vu;
  }
  const double dq[4] = {qw, s * ox, s * oy, s * oz};
  const double *q = pose;
  double nq[4] = {((dq[0] * q[0] - dq[1] * q[1]) - dq[2] * q[2]) - dq[3] * q[3], ((dq[0] * q[1] + dq[1] * q[0]) + dq[2] * q[3]) - dq[3] * q[2],
                  ((dq[0] * q[2] - dq[1] * q[3]) + dq[2] * q[0]) + dq[3] * q[1], ((dq[0] * q[3] + dq[1] * q[2]) - dq[2] * q[1]) + dq[3] * q[0]};
  const double sign = nq[0] < 0.0 ? -1.0 : 1.0;
  const double n = sqrt(((nq[0] * nq[0] + nq[1] * nq[1]) + nq[2] * nq[2]) + nq[3] * nq[3]);
  for (int i = 0; i < 4; i++) out[i] = sign * nq[i] / n;
  for (int i = 0; i < 3; i++) out[4 + i] = t[i];
}

// fixed-tree block reductions; `red` holds kThreads doubles; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double *red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double block_max(double v, double *red) {  // of non-negative values
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

template <bool kDepth>
__global__ __launch_bounds__(kThreads) void bundle_adjust_kernel(ArgsOf<kDepth> A) {
  constexpr int kRows = kDepth ? 3 : 2;
  __shared__ double S[kPacked];            // reduced system, lower triangle; then its Cholesky factor
  __shared__ double bp[kMaxN], xs[kMaxN], xsol[kMaxN];  // b of the poses; right-hand side (-> y of L y = rhs); the solution
  __shared__ double pose_lin[kMaxFree][7], pose_trial[kMaxFree][7];
  __shared__ double red[kThreads];
  __shared__ double tW[kTile][18], tY[kTile][18];  // per slot: W = w Jj^T Ji and Y = W (H_ll + lam)^-1, [6][3]
  __shared__ double tHinv[kTile][6], tbl[kTile][3];
  __shared__ uint32_t tmask[kTile];        // low 16 bits: free poses the point has an edge to (slot order); high 16: the active ones
  __shared__ int32_t tbase[kTile];         // the point's first slot

  const ProblemDev P = A.problems[blockIdx.x];
  const int tid = threadIdx.x;
  sdvl_bundle_result res;
  memset(&res, 0, sizeof(res));
  res.status = P.status;
  res.n_free = P.n_free;
  if (P.status != SDVL_BUNDLE_OK) {
    if (tid == 0) A.results[blockIdx.x] = res;
    return;
  }
  const EdgeDev *__restrict__ edges = A.edges;
  const int32_t *__restrict__ pt_off = A.pt_off + P.ptoff_begin, *__restrict__ pt_fe_off = A.pt_fe_off + P.ptoff_begin;
  const int32_t *__restrict__ kf_off = A.kf_off + P.kfoff_begin, *__restrict__ tile_pt = A.tile_pt + P.tile_begin;
  double *points = A.points + 3 * static_cast<size_t>(P.pt_begin), *pts_trial = A.pts_trial + 3 * static_cast<size_t>(P.pt_begin);
  double *ptblk = A.ptblk + 9 * static_cast<size_t>(P.pt_begin);
  double *rt_lin = A.rt_lin + 12 * static_cast<size_t>(P.kf_begin), *rt_trial = A.rt_trial + 12 * static_cast<size_t>(P.kf_begin);
  double *hpp = A.hpp + static_cast<size_t>(blockIdx.x) * kMaxFree * 36;
  double *hpart = A.hpart + static_cast<size_t>(blockIdx.x) * kMaxFree * 16 * 27;
  int32_t *levels = A.levels;
  auto edge_d = [&](int e) -> double {  // the measured depth of (absolute) edge e
    if constexpr (kDepth) return A.edge_depth[e];
    return 0.0;
  };
  const int nf = P.n_free, n = 6 * nf;
  const int n_items = items_of(nf);

  // the entries this thread owns: item -> (a, b, r, c) with a >= b, and c <= r when a == b; block row a begins at item
  // 36 a (a + 1) / 2 - 15 a and holds a full blocks and one triangle; the last n items are the right-hand side (b = -1); b = -2: none
  int item_a[kItems], item_b[kItems], item_r[kItems], item_c[kItems];
#pragma unroll
  for (int k = 0; k < kItems; k++) {
    const int item = tid + kThreads * k;
    int a = 0, b = -2, r = 0, c = 0;
    if (item < n_items - n) {
      while (18 * (a + 1) * (a + 2) - 15 * (a + 1) <= item) a++;
      const int rem = item - (18 * a * (a + 1) - 15 * a);
      if (rem < 36 * a) {
        b = rem / 36;
        r = (rem - 36 * b) / 6;
        c = rem - 36 * b - 6 * r;
      } else {
        const int t = rem - 36 * a;
        b = a;
        while ((r + 1) * (r + 2) / 2 <= t) r++;
        c = t - r * (r + 1) / 2;
      }
    } else if (item < n_items) {
      const int i = item - (n_items - n);
      a = i / 6;
      r = i - 6 * a;
      b = -1;
    }
    item_a[k] = a; item_b[k] = b; item_r[k] = r; item_c[k] = c;
  }

  for (int k = tid; k < P.n_kf; k += kThreads) {
    double rt[12];
    quat_to_rt(A.poses + 7 * static_cast<size_t>(P.kf_begin + k), rt);
    for (int i = 0; i < 12; i++) rt_lin[12 * k + i] = rt_trial[12 * k + i] = rt[i];
    if (k < nf)
      for (int i = 0; i < 7; i++) pose_lin[k][i] = A.poses[7 * static_cast<size_t>(P.kf_begin + k) + i];
    A.pose_stages[P.kf_begin + k] = 0;
  }
  for (int p = tid; p < P.n_pt; p += kThreads) A.point_stages[P.pt_begin + p] = 0;
  for (int e = tid; e < P.n_e; e += kThreads) levels[P.e_begin + e] = 0;
  __syncthreads();

  for (int stage = 0; stage < 2; stage++) {
    const bool robust = stage == 0;
    if (stage == 1) {
      // bundle.cc:196-205 at the accepted estimates: chi2 > 5.991 (a depth edge: 7.815) or depth not positive -> level 1
      double n1 = 0.0, n_free_active = 0.0;
      for (int e = tid; e < P.n_e; e += kThreads) {
        const EdgeDev ed = edges[P.e_begin + e];
        const double dm = edge_d(P.e_begin + e);
        const Geo g = edge_geo<kDepth>(rt_lin + 12 * ed.kf, points + 3 * ed.pt, ed.u, ed.v, dm, A);
        const bool bad = (edge_chi2<kDepth>(g) > edge_threshold<kDepth>(dm)) || !(g.z > 0.0);
        levels[P.e_begin + e] = bad ? 1 : 0;
        n1 += bad ? 1.0 : 0.0;
        n_free_active += (!bad && ed.kf < nf) ? 1.0 : 0.0;
      }
      res.n_level1 = static_cast<int32_t>(block_sum(n1, red));
      if (block_sum(n_free_active, red) == 0.0) break;  // nothing left to solve
    }
    // which vertices take part in this stage
    for (int p = tid; p < P.n_pt; p += kThreads) {
      bool any = false;
      for (int e = pt_off[p]; e < pt_off[p + 1]; e++) any = any || levels[e] == 0;
      if (any) A.point_stages[P.pt_begin + p] |= 1 << stage;
    }
    for (int k = tid; k < P.n_kf; k += kThreads) {
      bool any = false;
      for (int i = kf_off[k]; i < kf_off[k + 1]; i++) any = any || levels[A.kf_edges[i]] == 0;
      if (any) A.pose_stages[P.kf_begin + k] |= 1 << stage;
    }
    sdvl_bundle_stage &st = res.stage[stage];
    double lam = 0.0, ni = 2.0;
    int n_bad = 0;
    for (int it = 0; it < (stage == 0 ? 5 : 10); it++) {  // optimize(5), optimize(10): bundle.cc:193,209
      // ---- buildSystem at the linearisation point: H_ll, b_l and chi2 per point ...
      double chi_part = 0.0, diag_part = 0.0;
      for (int p = tid; p < P.n_pt; p += kThreads) {
        double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int e = pt_off[p]; e < pt_off[p + 1]; e++) {
          if (levels[e] != 0) continue;
          const EdgeDev ed = edges[e];
          const double *rt = rt_lin + 12 * ed.kf;
          const double dm = edge_d(e);
          const Geo g = edge_geo<kDepth>(rt, points + 3 * p, ed.u, ed.v, dm, A);
          double Ji[kRows][3], Jj[kRows][6], cost;
          edge_jacobians<kDepth>(g, rt, dm, A, Ji, Jj);
          const double w = huber(edge_chi2<kDepth>(g), robust, dm > 0.0, &cost);
          chi_part += cost;
          h[0] += w * rows_jj<kDepth>(Ji, 0, Ji, 0);
          h[1] += w * rows_jj<kDepth>(Ji, 0, Ji, 1);
          h[2] += w * rows_jj<kDepth>(Ji, 0, Ji, 2);
          h[3] += w * rows_jj<kDepth>(Ji, 1, Ji, 1);
          h[4] += w * rows_jj<kDepth>(Ji, 1, Ji, 2);
          h[5] += w * rows_jj<kDepth>(Ji, 2, Ji, 2);
          for (int c = 0; c < 3; c++) h[6 + c] += -w * rows_je<kDepth>(Ji, c, g);
        }
        for (int i = 0; i < 9; i++) ptblk[9 * p + i] = h[i];
        diag_part = fmax(diag_part, fmax(fabs(h[0]), fmax(fabs(h[3]), fabs(h[5]))));
      }
      // ... and H_pp, b_p per free pose over its keyframe-major list: 16 lanes per pose take every 16th edge of the list and keep the
      // 21 entries of the lower triangle and the 6 of b in registers; the 16 partial sums are added in lane order
      if ((tid >> 4) < nf) {
        const int a = tid >> 4, l = tid & 15;
        double acc[27];
        for (int k = 0; k < 27; k++) acc[k] = 0.0;
        for (int i = kf_off[a] + l; i < kf_off[a + 1]; i += 16) {
          const int e = A.kf_edges[i];
          if (levels[e] != 0) continue;
          const EdgeDev ed = edges[e];
          const double *rt = rt_lin + 12 * a;
          const double dm = edge_d(e);
          const Geo g = edge_geo<kDepth>(rt, points + 3 * ed.pt, ed.u, ed.v, dm, A);
          double Ji[kRows][3], Jj[kRows][6], cost;
          edge_jacobians<kDepth>(g, rt, dm, A, Ji, Jj);
          const double w = huber(edge_chi2<kDepth>(g), robust, dm > 0.0, &cost);
          for (int r = 0, k = 0; r < 6; r++) {
            for (int c = 0; c <= r; c++, k++) acc[k] += w * rows_jj<kDepth>(Jj, r, Jj, c);
            acc[21 + r] += -w * rows_je<kDepth>(Jj, r, g);
          }
        }
        for (int k = 0; k < 27; k++) hpart[(a * 16 + l) * 27 + k] = acc[k];
      }
      __syncthreads();
      for (int item = tid; item < nf * 27; item += kThreads) {
        const int a = item / 27, k = item - 27 * a;
        double acc = 0.0;
        for (int l = 0; l < 16; l++) acc += hpart[(a * 16 + l) * 27 + k];
        if (k < 21) {
          int r = 0;
          while ((r + 1) * (r + 2) / 2 <= k) r++;
          const int c = k - r * (r + 1) / 2;
          hpp[36 * a + 6 * r + c] = acc;
          hpp[36 * a + 6 * c + r] = acc;
          if (r == c) diag_part = fmax(diag_part, fabs(acc));
        } else {
          bp[6 * a + k - 21] = acc;
        }
      }
      double chi = block_sum(chi_part, red);
      const double max_diag = block_max(diag_part, red);
      if (it == 0) {
        st.chi2_before = st.chi2_after = chi;
        if (!isfinite(chi)) {
          res.status = SDVL_BUNDLE_NONFINITE;
          goto done;
        }
        lam = 1e-5 * max_diag;  // computeLambdaInit, optimization_algorithm_levenberg.cpp:166-180
        ni = 2.0;
        n_bad = 0;
      }
      const double chi0 = chi;
      int q = 0;
      double rho = 0.0;
      bool accepted = false;
      do {
        // ---- the reduced system S = H_pp + lam - sum_p W_p (H_ll + lam)^-1 W_p^T and its right-hand side, tile by tile
        double acc[kItems];
#pragma unroll
        for (int k = 0; k < kItems; k++) acc[k] = 0.0;
        for (int t = 0; t < P.n_tiles; t++) {
          const int p0 = tile_pt[t], np = tile_pt[t + 1] - p0;
          const int slot0 = pt_fe_off[p0];
          if (tid < np) {
            const int p = p0 + tid;
            uint32_t m = 0;
            for (int i = pt_fe_off[p]; i < pt_fe_off[p + 1]; i++) {
              const int e = A.fe[i];
              m |= (1u << edges[e].kf) | (levels[e] == 0 ? 0x10000u << edges[e].kf : 0u);
            }
            tmask[tid] = m;
            tbase[tid] = pt_fe_off[p] - slot0;
            inv3_sym(ptblk + 9 * p, lam, tHinv[tid]);
            for (int c = 0; c < 3; c++) tbl[tid][c] = ptblk[9 * p + 6 + c];
          }
          __syncthreads();
          const int n_slots = pt_fe_off[p0 + np] - slot0;
          if (tid < n_slots) {
            const int e = A.fe[slot0 + tid];
            const EdgeDev ed = edges[e];
            if (levels[e] == 0) {
              const double *rt = rt_lin + 12 * ed.kf;
              const double dm = edge_d(e);
              const Geo g = edge_geo<kDepth>(rt, points + 3 * ed.pt, ed.u, ed.v, dm, A);
              double Ji[kRows][3], Jj[kRows][6], cost;
              edge_jacobians<kDepth>(g, rt, dm, A, Ji, Jj);
              const double w = huber(edge_chi2<kDepth>(g), robust, dm > 0.0, &cost);
              const double *hi = tHinv[ed.pt - p0];
              const double H3[3][3] = {{hi[0], hi[1], hi[2]}, {hi[1], hi[3], hi[4]}, {hi[2], hi[4], hi[5]}};
              for (int i = 0; i < 6; i++) {
                double wr[3];
                for (int c = 0; c < 3; c++) wr[c] = w * rows_jj<kDepth>(Jj, i, Ji, c);
                for (int c = 0; c < 3; c++) {
                  tW[tid][3 * i + c] = wr[c];
                  tY[tid][3 * i + c] = (wr[0] * H3[0][c] + wr[1] * H3[1][c]) + wr[2] * H3[2][c];
                }
              }
            }
          }
          __syncthreads();
          for (int pp = 0; pp < np; pp++) {
            const uint32_t m = tmask[pp], act = m >> 16;
            const int base = tbase[pp];
#pragma unroll
            for (int k = 0; k < kItems; k++) {
              const int a = item_a[k], b = item_b[k];
              if (b == -2 || !((act >> a) & 1u)) continue;
              const double *y = tY[base + __popc(m & 0xffffu & ((1u << a) - 1u))] + 3 * item_r[k];
              if (b == -1) {
                acc[k] += (y[0] * tbl[pp][0] + y[1] * tbl[pp][1]) + y[2] * tbl[pp][2];
              } else if ((act >> b) & 1u) {
                const double *w = tW[base + __popc(m & 0xffffu & ((1u << b) - 1u))] + 3 * item_c[k];
                acc[k] += (y[0] * w[0] + y[1] * w[1]) + y[2] * w[2];
              }
            }
          }
          __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < kItems; k++) {
          const int a = item_a[k], b = item_b[k], r = item_r[k], c = item_c[k];
          if (b == -1) {
            xs[6 * a + r] = bp[6 * a + r] - acc[k];
          } else if (b >= 0) {
            const double hv = a == b ? hpp[36 * a + 6 * r + c] + (r == c ? lam : 0.0) : 0.0;
            S[tri(6 * a + r, 6 * b + c)] = hv - acc[k];
          }
        }
        // ---- dense column Cholesky in place (LinearSolverEigen's LL^T restated as dense); a pivot that is not > 0 fails the solve.
        // The right-hand side rides along as row n of the matrix, which is the forward substitution L y = rhs.  One barrier per
        // column: the trailing update of column k reads column k unscaled (dividing by the pivot's root as it goes); the scaled
        // column k is stored after the next barrier, beside the update of column k + 1, which never reads it.
        // Invariant behind the barrier at the top of iteration k: columns 0 .. k - 2 are final (scaled L); column k - 1 has all its
        // trailing updates but is still unscaled, with its pivot's root in sd_prev; columns k .. n - 1 hold the Schur complement of the
        // first k columns.  The iteration scales column k - 1 (rows >= k; the diagonal gets sd_prev) and updates columns k + 1 .. from
        // column k alone, so the two writes never touch what the other reads.  The pivot d is read from LDS behind the barrier by every
        // thread alike: the break is taken by the whole workgroup.
        auto M = [&](int i, int j) -> double & { return i == n ? xs[j] : S[tri(i, j)]; };
        bool ok = true;
        double sd_prev = 1.0;
        for (int k = 0; k <= n; k++) {
          __syncthreads();
          if (k > 0) {  // column k - 1, scaled
            if (tid == 0) S[tri(k - 1, k - 1)] = sd_prev;
            for (int i = k + tid; i <= n; i += kThreads) M(i, k - 1) = M(i, k - 1) / sd_prev;
          }
          if (k == n) break;
          const double d = S[tri(k, k)];
          if (!(d > 0.0) || !isfinite(d)) {
            ok = false;
            break;
          }
          const double sd = sqrt(d);
          for (int i = k + 1 + (tid >> 5); i <= n; i += kThreads / 32) {
            const double lik = M(i, k) / sd;
            for (int j = k + 1 + (tid & 31); j <= i && j < n; j += 32) M(i, j) = M(i, j) - lik * (S[tri(j, k)] / sd);
          }
          sd_prev = sd;
        }
        __syncthreads();
        double chi_new = DBL_MAX, scale = 0.0;
        if (ok) {
          for (int k = n - 1; k >= 0; k--) {  // L^T x = y: xs[k] is final when step k reads it; the solution goes to xsol
            const double xk = xs[k] / S[tri(k, k)];
            if (tid == k) xsol[k] = xk;
            if (tid < k) xs[tid] = xs[tid] - S[tri(k, tid)] * xk;
            __syncthreads();
          }
          // ---- the trial estimates: poses exp(x) T, points X + (H_ll + lam)^-1 (b_l - W^T x); computeScale (:182-189)
          double scale_part = 0.0;
          if (tid < nf) {
            exp_update(pose_lin[tid], xsol + 6 * tid, pose_trial[tid]);
            quat_to_rt(pose_trial[tid], rt_trial + 12 * tid);
          }
          if (tid < n) scale_part += xsol[tid] * (lam * xsol[tid] + bp[tid]);
          for (int p = tid; p < P.n_pt; p += kThreads) {
            double hi[6], tv[3] = {ptblk[9 * p + 6], ptblk[9 * p + 7], ptblk[9 * p + 8]};
            const double bl[3] = {tv[0], tv[1], tv[2]};
            inv3_sym(ptblk + 9 * p, lam, hi);
            for (int i = pt_fe_off[p]; i < pt_fe_off[p + 1]; i++) {
              const int e = A.fe[i];
              if (levels[e] != 0) continue;
              const EdgeDev ed = edges[e];
              const double *rt = rt_lin + 12 * ed.kf;
              const double dm = edge_d(e);
              const Geo g = edge_geo<kDepth>(rt, points + 3 * p, ed.u, ed.v, dm, A);
              double Ji[kRows][3], Jj[kRows][6], cost;
              edge_jacobians<kDepth>(g, rt, dm, A, Ji, Jj);
              const double w = huber(edge_chi2<kDepth>(g), robust, dm > 0.0, &cost);
              const double *xa = xsol + 6 * ed.kf;
              for (int c = 0; c < 3; c++) {
                double s = 0.0;
                for (int r = 0; r < 6; r++) s += w * rows_jj<kDepth>(Jj, r, Ji, c) * xa[r];
                tv[c] -= s;
              }
            }
            const double dl[3] = {(hi[0] * tv[0] + hi[1] * tv[1]) + hi[2] * tv[2], (hi[1] * tv[0] + hi[3] * tv[1]) + hi[4] * tv[2],
                                  (hi[2] * tv[0] + hi[4] * tv[1]) + hi[5] * tv[2]};
            for (int c = 0; c < 3; c++) {
              pts_trial[3 * p + c] = points[3 * p + c] + dl[c];
              scale_part += dl[c] * (lam * dl[c] + bl[c]);
            }
          }
          scale = block_sum(scale_part, red);  // the barriers inside also publish the trial estimates
          // ---- computeActiveErrors + activeRobustChi2 at the trial
          double cpart = 0.0;
          for (int p = tid; p < P.n_pt; p += kThreads)
            for (int e = pt_off[p]; e < pt_off[p + 1]; e++) {
              if (levels[e] != 0) continue;
              const EdgeDev ed = edges[e];
              const double dm = edge_d(e);
              const Geo g = edge_geo<kDepth>(rt_trial + 12 * ed.kf, pts_trial + 3 * p, ed.u, ed.v, dm, A);
              double cost;
              huber(edge_chi2<kDepth>(g), robust, dm > 0.0, &cost);
              cpart += cost;
            }
          chi_new = block_sum(cpart, red);
          rho = (chi - chi_new) / (scale + 1e-3);
          accepted = rho > 0.0 && isfinite(chi_new);
        } else {
          rho = -INFINITY;  // a failed solve is a rejected trial
          accepted = false;
        }
        if (accepted) {
          const double tq = 2.0 * rho - 1.0;
          lam *= fmax(1.0 / 3.0, fmin(2.0 / 3.0, 1.0 - tq * tq * tq));
          ni = 2.0;
          chi = chi_new;
          if (tid < nf) {
            for (int i = 0; i < 7; i++) pose_lin[tid][i] = pose_trial[tid][i];
            for (int i = 0; i < 12; i++) rt_lin[12 * tid + i] = rt_trial[12 * tid + i];
          }
          for (int i = tid; i < 3 * P.n_pt; i += kThreads) points[i] = pts_trial[i];
        } else {
          lam *= ni;
          ni *= 2.0;
        }
        __syncthreads();
        q++;
      } while (rho < 0.0 && q < kMaxTrials);
      st.iterations++;
      st.trials += q;
      st.trials_per_it[it] = q;
      if (accepted) st.accepted_mask |= 1 << it;
      st.chi2_after = chi;
      st.lambda = lam;
      if (q == kMaxTrials || rho == 0.0) break;
      n_bad = (chi0 - chi) * 1e3 < chi0 ? n_bad + 1 : 0;
      if (n_bad >= 3) break;
    }
  }
  if (tid < nf)
    for (int i = 0; i < 7; i++) A.poses[7 * static_cast<size_t>(P.kf_begin + tid) + i] = pose_lin[tid][i];
done:
  if (tid == 0) A.results[blockIdx.x] = res;
}

inline double depth_of(const sdvl_bundle_edge &) { return 0.0; }
inline double depth_of(const sdvl_bundle_edge_depth &e) { return e.depth; }

// Both entry points.  Edge = sdvl_bundle_edge: the monocular kernel over every problem, one launch.  Edge = sdvl_bundle_edge_depth:
// the problems none of whose edges carries a depth are listed first and go to the monocular kernel as they are, which is what gives
// them the monocular call's bits whatever their neighbours carry; the others go to the depth form in a second launch.
template <class Edge>
int bundle_adjust_any(sdvl_ctx *ctx, int n_problems, const sdvl_bundle_problem *problems, int n_kf, double *poses, const int32_t *fixed, int n_pt,
                      double *points, int n_e, const Edge *edges, const sdvl_camera *cam, double bf, int32_t *edge_levels, int32_t *pose_stages,
                      int32_t *point_stages, sdvl_bundle_result *results) {
  constexpr bool kDepthCall = std::is_same<Edge, sdvl_bundle_edge_depth>::value;
  if (!ctx || !cam || n_problems < 0 || n_kf < 0 || n_pt < 0 || n_e < 0 || (n_problems > 0 && (!problems || !results)) ||
      (n_kf > 0 && (!poses || !fixed || !pose_stages)) || (n_pt > 0 && (!points || !point_stages)) || (n_e > 0 && (!edges || !edge_levels)))
    return SDVL_ERR_INVALID;
  if (n_problems == 0) return SDVL_OK;
  // ---- checks first: nothing is written before every problem has passed
  std::vector<ProblemDev> pd(n_problems);
  std::vector<char> with_depth(n_problems, 0);
  size_t n_ptoff = 0, n_kfoff = 0, n_fe = 0;
  int prev_kf = 0, prev_pt = 0, prev_e = 0;
  if (kDepthCall) {
    bool any = false;
    for (int j = 0; j < n_problems; j++)
      for (int e = std::max(problems[j].edge_begin, 0); e < std::min(problems[j].edge_end, n_e); e++) {
        const double d = depth_of(edges[e]);
        SDVL_REQUIRE(ctx, std::isfinite(d), "an edge's depth is NaN or infinite (<= 0 means none)");
        if (d > 0.0) with_depth[j] = 1, any = true;
      }
    SDVL_REQUIRE(ctx, !any || (std::isfinite(bf) && bf > 0.0), "bf must be finite and > 0 when an edge carries a depth");
  }
  for (int j = 0; j < n_problems; j++) {
    const sdvl_bundle_problem &a = problems[j];
    SDVL_REQUIRE(ctx, a.kf_begin >= prev_kf && a.kf_end >= a.kf_begin && a.kf_end <= n_kf, "pose range out of bounds or overlapping");
    SDVL_REQUIRE(ctx, a.pt_begin >= prev_pt && a.pt_end >= a.pt_begin && a.pt_end <= n_pt, "point range out of bounds or overlapping");
    SDVL_REQUIRE(ctx, a.edge_begin >= prev_e && a.edge_end >= a.edge_begin && a.edge_end <= n_e, "edge range out of bounds or overlapping");
    prev_kf = a.kf_end; prev_pt = a.pt_end; prev_e = a.edge_end;
    ProblemDev &p = pd[j];
    p = ProblemDev{a.kf_begin, a.kf_end - a.kf_begin, 0, a.pt_begin, a.pt_end - a.pt_begin, a.edge_begin, a.edge_end - a.edge_begin, 0, 0, 0, 0, SDVL_BUNDLE_OK};
    while (p.n_free < p.n_kf && !fixed[a.kf_begin + p.n_free]) p.n_free++;
    for (int k = p.n_free; k < p.n_kf; k++) SDVL_REQUIRE(ctx, fixed[a.kf_begin + k], "the free poses of a problem come first");
    if (p.n_free > kMaxFree) {
      ctx->err = "more than SDVL_BUNDLE_MAX_FREE free poses in one bundle problem";
      return SDVL_ERR_CAPACITY;
    }
    int free_edges = 0;
    for (int e = a.edge_begin; e < a.edge_end; e++) {
      SDVL_REQUIRE(ctx, edges[e].point >= 0 && edges[e].point < p.n_pt && edges[e].keyframe >= 0 && edges[e].keyframe < p.n_kf,
                   "edge names a point or a pose outside its problem");
      free_edges += edges[e].keyframe < p.n_free ? 1 : 0;
    }
    if (p.n_kf == 0 || p.n_pt == 0) p.status = SDVL_BUNDLE_EMPTY;
    else if (free_edges == 0) p.status = SDVL_BUNDLE_NO_EDGES;
    p.ptoff_begin = static_cast<int32_t>(n_ptoff);
    p.kfoff_begin = static_cast<int32_t>(n_kfoff);
    n_ptoff += static_cast<size_t>(p.n_pt) + 1;
    n_kfoff += static_cast<size_t>(p.n_kf) + 1;
    n_fe += static_cast<size_t>(free_edges);
  }
  // ---- the two indices: edges point-major (then by pose), the keyframe-major list, the edges to free poses, the Schur tiles
  std::vector<int32_t> order(std::max(n_e, 1)), pt_off(n_ptoff), pt_fe_off(n_ptoff), kf_off(n_kfoff), kf_edges(std::max(n_e, 1)), fe(std::max<size_t>(n_fe, 1)), tile_pt;
  std::vector<int32_t> csr_of(std::max(n_e, 1), -1);  // caller's edge -> CSR position; -1: an edge of no problem
  size_t at = 0, fe_at = 0;
  for (int j = 0; j < n_problems; j++) {
    ProblemDev &p = pd[j];
    const int e0 = p.e_begin;
    int32_t *ord = order.data() + at;
    std::iota(ord, ord + p.n_e, e0);
    std::stable_sort(ord, ord + p.n_e, [&](int32_t x, int32_t y) {
      return edges[x].point != edges[y].point ? edges[x].point < edges[y].point : edges[x].keyframe < edges[y].keyframe;
    });
    for (int i = 1; i < p.n_e; i++)
      SDVL_REQUIRE(ctx, edges[ord[i]].point != edges[ord[i - 1]].point || edges[ord[i]].keyframe != edges[ord[i - 1]].keyframe,
                   "two edges between the same point and pose");
    int32_t *po = pt_off.data() + p.ptoff_begin, *pf = pt_fe_off.data() + p.ptoff_begin, *ko = kf_off.data() + p.kfoff_begin;
    std::fill(ko, ko + p.n_kf + 1, 0);
    int i = 0;
    for (int q = 0; q < p.n_pt; q++) {
      po[q] = static_cast<int32_t>(at) + i;
      pf[q] = static_cast<int32_t>(fe_at);
      for (; i < p.n_e && edges[ord[i]].point == q; i++) {
        csr_of[ord[i]] = static_cast<int32_t>(at) + i;
        ko[edges[ord[i]].keyframe + 1]++;
        if (edges[ord[i]].keyframe < p.n_free) fe[fe_at++] = static_cast<int32_t>(at) + i;
      }
    }
    po[p.n_pt] = static_cast<int32_t>(at) + p.n_e;
    pf[p.n_pt] = static_cast<int32_t>(fe_at);
    for (int k = 0; k < p.n_kf; k++) ko[k + 1] += ko[k];
    std::vector<int32_t> fill(ko, ko + p.n_kf);
    for (int c = 0; c < p.n_e; c++) kf_edges[at + fill[edges[ord[c]].keyframe]++] = static_cast<int32_t>(at) + c;
    for (int k = 0; k <= p.n_kf; k++) ko[k] += static_cast<int32_t>(at);
    // tiles: consecutive points while their free edges fit kTile slots (a point has at most kMaxFree <= kTile of them)
    p.tile_begin = static_cast<int32_t>(tile_pt.size());
    tile_pt.push_back(0);
    for (int q = 0, first = 0; q < p.n_pt; q++) {
      if (pf[q + 1] - pf[first] > kTile || q + 1 - first > kTile) {
        tile_pt.push_back(q);
        first = q;
      }
      if (q == p.n_pt - 1) tile_pt.push_back(p.n_pt);
    }
    p.n_tiles = static_cast<int32_t>(tile_pt.size()) - p.tile_begin - 1;
    p.e_begin = static_cast<int32_t>(at);
    at += static_cast<size_t>(p.n_e);
  }
  const size_t n_csr = at;
  sdvl_layout st, o, wk;  // staging: everything the kernel reads; d_out / h_out: what returns; d_work: scratch
  const sdvl_part<ProblemDev> st_prob = st.take<ProblemDev>(n_problems);
  const sdvl_part<EdgeDev> st_edges = st.take<EdgeDev>(std::max<size_t>(n_csr, 1));
  const sdvl_part<int32_t> st_ptoff = st.take<int32_t>(n_ptoff), st_ptfe = st.take<int32_t>(n_ptoff), st_kfoff = st.take<int32_t>(n_kfoff);
  const sdvl_part<int32_t> st_kfe = st.take<int32_t>(std::max<size_t>(n_csr, 1)), st_fe = st.take<int32_t>(fe.size()), st_tile = st.take<int32_t>(tile_pt.size());
  const sdvl_part<double> st_poses = st.take<double>(7 * static_cast<size_t>(std::max(n_kf, 1))), st_points = st.take<double>(3 * static_cast<size_t>(std::max(n_pt, 1)));
  const sdvl_part<double> st_depth = kDepthCall ? st.take<double>(std::max<size_t>(n_csr, 1)) : sdvl_part<double>{};
  const sdvl_part<double> o_poses = o.take<double>(st_poses.count), o_points = o.take<double>(st_points.count);
  const sdvl_part<int32_t> o_levels = o.take<int32_t>(std::max<size_t>(n_csr, 1)), o_pstage = o.take<int32_t>(std::max(n_kf, 1)), o_qstage = o.take<int32_t>(std::max(n_pt, 1));
  const sdvl_part<sdvl_bundle_result> o_res = o.take<sdvl_bundle_result>(n_problems);
  const sdvl_part<double> wk_trial = wk.take<double>(st_points.count), wk_blk = wk.take<double>(9 * static_cast<size_t>(std::max(n_pt, 1)));
  const sdvl_part<double> wk_rtl = wk.take<double>(12 * static_cast<size_t>(std::max(n_kf, 1))), wk_rtt = wk.take<double>(12 * static_cast<size_t>(std::max(n_kf, 1)));
  const sdvl_part<double> wk_hpp = wk.take<double>(static_cast<size_t>(n_problems) * kMaxFree * 36);
  const sdvl_part<double> wk_hpart = wk.take<double>(static_cast<size_t>(n_problems) * kMaxFree * 16 * 27);
  void *hs = nullptr, *dsx = nullptr;
  int rc = sdvl_ensure(ctx, &ctx->d_work, &ctx->d_work_bytes, wk.bytes(), false);
  if (!rc) rc = sdvl_ensure(ctx, &ctx->d_out, &ctx->d_out_bytes, o.bytes(), false);
  if (!rc) rc = sdvl_ensure(ctx, &ctx->h_out, &ctx->h_out_bytes, o.bytes(), true);
  if (!rc) rc = sdvl_stage_alloc(ctx, st.bytes(), &hs, &dsx);
  if (rc) return rc;
  // the kernels' problem lists: the problems without a depth first (all of them in the monocular call), in the caller's order
  std::vector<int32_t> perm;
  for (int pass = 0; pass < 2; pass++)
    for (int j = 0; j < n_problems; j++)
      if (with_depth[j] == pass) perm.push_back(j);
  const int n_mono = static_cast<int>(std::count(with_depth.begin(), with_depth.end(), 0));
  for (int i = 0; i < n_problems; i++) st_prob.in(hs)[i] = pd[perm[i]];
  EdgeDev *he = st_edges.in(hs);
  for (size_t c = 0; c < n_csr; c++) {
    const Edge &e = edges[order[c]];
    he[c] = EdgeDev{e.point, e.keyframe, e.u, e.v};
    if (kDepthCall) st_depth.in(hs)[c] = depth_of(e);
  }
  memcpy(st_ptoff.in(hs), pt_off.data(), st_ptoff.bytes());
  memcpy(st_ptfe.in(hs), pt_fe_off.data(), st_ptfe.bytes());
  memcpy(st_kfoff.in(hs), kf_off.data(), st_kfoff.bytes());
  memcpy(st_kfe.in(hs), kf_edges.data(), sizeof(int32_t) * n_csr);
  memcpy(st_fe.in(hs), fe.data(), st_fe.bytes());
  memcpy(st_tile.in(hs), tile_pt.data(), st_tile.bytes());
  if (n_kf) memcpy(st_poses.in(hs), poses, sizeof(double) * 7 * static_cast<size_t>(n_kf));
  if (n_pt) memcpy(st_points.in(hs), points, sizeof(double) * 3 * static_cast<size_t>(n_pt));
  SDVL_HIP_CHECK(ctx, sdvl_push(ctx, dsx, hs, st.bytes()));
  // the kernel updates poses and points in place in d_out: seed them from the staged copy
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(o_poses.in(ctx->d_out), st_poses.cin(dsx), o_poses.bytes(), hipMemcpyDeviceToDevice, ctx->stream));
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(o_points.in(ctx->d_out), st_points.cin(dsx), o_points.bytes(), hipMemcpyDeviceToDevice, ctx->stream));
  BundleArgs A;
  A.problems = st_prob.cin(dsx);
  A.edges = st_edges.cin(dsx);
  A.pt_off = st_ptoff.cin(dsx);
  A.kf_off = st_kfoff.cin(dsx);
  A.kf_edges = st_kfe.cin(dsx);
  A.pt_fe_off = st_ptfe.cin(dsx);
  A.fe = st_fe.cin(dsx);
  A.tile_pt = st_tile.cin(dsx);
  A.poses = o_poses.in(ctx->d_out);
  A.points = o_points.in(ctx->d_out);
  A.pts_trial = wk_trial.in(ctx->d_work);
  A.ptblk = wk_blk.in(ctx->d_work);
  A.rt_lin = wk_rtl.in(ctx->d_work);
  A.rt_trial = wk_rtt.in(ctx->d_work);
  A.hpp = wk_hpp.in(ctx->d_work);
  A.hpart = wk_hpart.in(ctx->d_work);
  A.levels = o_levels.in(ctx->d_out);
  A.pose_stages = o_pstage.in(ctx->d_out);
  A.point_stages = o_qstage.in(ctx->d_out);
  A.results = o_res.in(ctx->d_out);
  A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->u0; A.cy = cam->v0;
  // vertices and edges of no problem keep zeros
  SDVL_HIP_CHECK(ctx, hipMemsetAsync(o_levels.in(ctx->d_out), 0, o.bytes() - o_levels.off, ctx->stream));
  if (n_mono > 0) SDVL_LAUNCH(ctx, "bundle_adjust", bundle_adjust_kernel<false>, dim3(n_mono), dim3(kThreads), A);
  if (n_mono < n_problems) {  // blockIdx.x counts from the first problem with a depth
    BundleArgsD D;
    static_cast<BundleArgs &>(D) = A;
    D.problems += n_mono;
    D.results += n_mono;
    D.hpp += static_cast<size_t>(n_mono) * kMaxFree * 36;
    D.hpart += static_cast<size_t>(n_mono) * kMaxFree * 16 * 27;
    D.edge_depth = st_depth.cin(dsx);
    D.bf = bf;
    SDVL_LAUNCH(ctx, "bundle_adjust_depth", bundle_adjust_kernel<true>, dim3(n_problems - n_mono), dim3(kThreads), D);
  }
  SDVL_HIP_CHECK(ctx, hipGetLastError());
  SDVL_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, o.bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SDVL_HIP_CHECK(ctx, sdvl_stream_wait(ctx));
  // ---- back to the caller: a problem that did not end SDVL_BUNDLE_OK leaves its poses, points and levels as they were given
  const sdvl_bundle_result *hr = o_res.cin(ctx->h_out);
  const double *hp = o_poses.cin(ctx->h_out), *hq = o_points.cin(ctx->h_out);
  const int32_t *hl = o_levels.cin(ctx->h_out);
  for (int i = 0; i < n_problems; i++) results[perm[i]] = hr[i];
  for (int e = 0; e < n_e; e++) edge_levels[e] = 0;
  for (int k = 0; k < n_kf; k++) pose_stages[k] = 0;
  for (int q = 0; q < n_pt; q++) point_stages[q] = 0;
  for (int j = 0; j < n_problems; j++) {
    if (results[j].status != SDVL_BUNDLE_OK) continue;
    const sdvl_bundle_problem &a = problems[j];
    memcpy(poses + 7 * static_cast<size_t>(a.kf_begin), hp + 7 * static_cast<size_t>(a.kf_begin), sizeof(double) * 7 * static_cast<size_t>(results[j].n_free));
    memcpy(points + 3 * static_cast<size_t>(a.pt_begin), hq + 3 * static_cast<size_t>(a.pt_begin), sizeof(double) * 3 * static_cast<size_t>(a.pt_end - a.pt_begin));
    for (int e = a.edge_begin; e < a.edge_end; e++) edge_levels[e] = hl[csr_of[e]];
    memcpy(pose_stages + a.kf_begin, o_pstage.cin(ctx->h_out) + a.kf_begin, sizeof(int32_t) * static_cast<size_t>(a.kf_end - a.kf_begin));
    memcpy(point_stages + a.pt_begin, o_qstage.cin(ctx->h_out) + a.pt_begin, sizeof(int32_t) * static_cast<size_t>(a.pt_end - a.pt_begin));
  }
  return SDVL_OK;
}

}  // namespace

extern "C" int sdvl_bundle_adjust(sdvl_ctx *ctx, int n_problems, const sdvl_bundle_problem *problems, int n_kf, double *poses, const int32_t *fixed,
                                  int n_pt, double *points, int n_e, const sdvl_bundle_edge *edges, const sdvl_camera *cam, int32_t *edge_levels,
                                  int32_t *pose_stages, int32_t *point_stages, sdvl_bundle_result *results) {
  return bundle_adjust_any(ctx, n_problems, problems, n_kf, poses, fixed, n_pt, points, n_e, edges, cam, 0.0, edge_levels, pose_stages, point_stages, results);
}

extern "C" int sdvl_bundle_adjust_depth(sdvl_ctx *ctx, int n_problems, const sdvl_bundle_problem *problems, int n_kf, double *poses, const int32_t *fixed,
                                        int n_pt, double *points, int n_e, const sdvl_bundle_edge_depth *edges, const sdvl_camera *cam, double bf,
                                        int32_t *edge_levels, int32_t *pose_stages, int32_t *point_stages, sdvl_bundle_result *results) {
  return bundle_adjust_any(ctx, n_problems, problems, n_kf, poses, fixed, n_pt, points, n_e, edges, cam, bf, edge_levels, pose_stages, point_stages, results);
}
