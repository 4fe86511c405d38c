// Batched RANSAC triangulation with Huber refinement, and the batched reprojection error,
// for gfx950.
//
// Replaces the host loop of mvn/models/triangulation.py:54-128 (RANSACTriangulationNet's
// triangulate_ransac over B x J) and mvn/utils/multiview.py:177-184
// (calc_reprojection_error_matrix).
//
// ransac_kernel: one 16-lane group owns one (b, j), four points per wave.
//   1. lane h of the group runs hypotheses h, h + 16, ... of the caller's pair list: the 4x4
//      system of the pair's two views (f64 rows pt * P[2] - P[0|1], multiview.py:119-122),
//      its null vector (dlt_solver.hpp), the half pixel distance of that point in every view
//      (multiview.py:177-184) and the inlier mask (the pair, plus every view with error <
//      epsilon, triangulation.py:90-94);
//   2. the group reduces (most inliers, then lowest hypothesis index) with four xor shuffles
//      inside its 16 lanes: no LDS, no atomics (triangulation.py:96-97 keeps the first set
//      of the largest size);
//   3. every lane of the group then runs the same unweighted DLT over the inlier views and,
//      if asked, the damped Gauss-Newton minimisation of the reference's Huber cost
//      (triangulation.py:115-124) -- redundantly, which costs one lane's latency and no
//      divergence -- and lane 0 stores the results.
#include "common.hpp"
#include "dlt_solver.hpp"

namespace mvn {
namespace {

constexpr int kRansacGroup = 16;                       // lanes per (b, j)
constexpr int kRansacBlock = 64;                       // one wave: four points
constexpr int kRansacPoints = kRansacBlock / kRansacGroup;
constexpr int kRansacMaxViews = 32;                    // the inlier set is a 32-bit mask
constexpr int kRansacMaxIters = 4096;
constexpr int kRefineTrials = 96;                      // cap on cost evaluations of the refinement

// Rows pt_x * P[2] - P[0] and pt_y * P[2] - P[1] of one view, in f64 from the f32 inputs
// (multiview.py:121-122 on numpy's f64 promotion: a product and a difference, each rounded),
// folded into R.
__device__ __forceinline__ void fold_view(double (&R)[4][4], const float* __restrict__ Pv, float px, float py) {
  const double pt[2] = {double(px), double(py)};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = pt[r] * double(Pv[8 + k]) - double(Pv[r * 4 + k]);
    givens_fold(R, a);
  }
}

// Null vector of R as dlt_kernel takes it (dlt_solver.hpp null_vector: exact zero column, inverse
// iteration, Jacobi SVD), dehomogenised (multiview.py:125-127).
__device__ __forceinline__ void solve_point(double (&R)[4][4], double (&x)[3]) {
  double X[4];
  null_vector(R, X);
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = X[i] / X[3];
}

// Projection of x through one view: the residual e = (pt - proj(x)) / 2 (its norm is the
// reference's reprojection error, multiview.py:180-181) and the homogeneous row products.
struct Proj {
  double e[2];      // half pixel residual
  double u[2];      // projected pixel
  double wi;        // 1 / depth
};
// kFast (the refinement's inner loop, a serial f64 chain): the depth's Newton-refined reciprocal
// (dlt_solver.hpp) and two products instead of three IEEE divisions.
template <bool kFast = false>
__device__ __forceinline__ Proj project(const float* __restrict__ Pv, float px, float py, const double (&x)[3]) {
  double h[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    h[r] = double(Pv[r * 4 + 0]) * x[0] + double(Pv[r * 4 + 1]) * x[1] + double(Pv[r * 4 + 2]) * x[2] +
           double(Pv[r * 4 + 3]);
  Proj p;
  if (kFast) {
    p.wi = rcp_nr(h[2]);
    p.u[0] = h[0] * p.wi;
    p.u[1] = h[1] * p.wi;
  } else {
    p.wi = 1.0 / h[2];
    p.u[0] = h[0] / h[2];
    p.u[1] = h[1] / h[2];
  }
  p.e[0] = 0.5 * (double(px) - p.u[0]);
  p.e[1] = 0.5 * (double(py) - p.u[1]);
  return p;
}
__device__ __forceinline__ double half_distance(const Proj& p) {
  return sqrt(p.e[0] * p.e[0] + p.e[1] * p.e[1]);
}

// The reference's cost at x over the views of `mask`: 1/2 sum rho(r_v^2), rho scipy's Huber
// with f_scale 1 (rho(z) = z for z <= 1, else 2 sqrt(z) - 1), with the gradient
// g = sum rho' J^T e and the Gauss-Newton matrix H = sum rho' J^T J + 2 rho'' (J^T e)(J^T e)^T
// (J = de/dx, 2x3; the second term is the exact curvature of the Huber tail and keeps H
// positive semi-definite: for z > 1 the view contributes (J^T J - q q^T / z) / r, q = J^T e).
// H is stored as its upper triangle xx, xy, xz, yy, yz, zz.
__device__ __forceinline__ double huber_cost(const float* __restrict__ Pb, const float* __restrict__ ptb, int J, int N,
                                             uint32_t mask, const double (&x)[3], double (&g)[3], double (&H)[6]) {
  double cost = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) H[i] = 0.0;
  for (int v = 0; v < N; ++v) {
    if (!((mask >> v) & 1u)) continue;
    const float* Pv = Pb + size_t(v) * 12;
    const float* pt = ptb + size_t(v) * J * 2;
    const Proj p = project<true>(Pv, pt[0], pt[1], x);
    const double z = p.e[0] * p.e[0] + p.e[1] * p.e[1];
    const bool tail = z > 1.0;
    const double ri = rsqrt_nr(tail ? z : 1.0);          // 1 / r where the tail needs it
    cost += tail ? 2.0 * (z * ri) - 1.0 : z;
    // J[c][k] = d e_c / d x_k = -(P[c][k] - u_c P[2][k]) / (2 w)
    double Jm[2][3];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        Jm[c][k] = -0.5 * p.wi * (double(Pv[c * 4 + k]) - p.u[c] * double(Pv[8 + k]));
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = Jm[0][k] * p.e[0] + Jm[1][k] * p.e[1];
    const double w1 = tail ? ri : 1.0;                 // rho'
    const double w2 = tail ? ri * ri * ri : 0.0;       // -2 rho''
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += w1 * q[k];
    int n = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = a; c < 3; ++c, ++n)
        H[n] += w1 * (Jm[0][a] * Jm[0][c] + Jm[1][a] * Jm[1][c]) - w2 * q[a] * q[c];
  }
  return 0.5 * cost;
}

// Levenberg-Marquardt on the cost above from x (the DLT point), in place.  Each trial solves
// (H + lambda diag(H)) d = -g by the adjugate (3x3, registers) and is accepted only if the
// cost does not rise (lambda / 5), otherwise lambda * 10 (lambda starts at 1e-2).  Deterministic
// stopping rule: a trial step with |d| <= 1e-9 |x| (accepted or not), a rejected trial whose cost
// is within 1e-14 (relative) of the current one, a zero gradient, lambda > 1e12, or kRefineTrials
// trials.  A non-finite start is returned as it is.
__device__ __forceinline__ void refine(const float* __restrict__ Pb, const float* __restrict__ ptb, int J, int N,
                                       uint32_t mask, double (&x)[3]) {
  double g[3], H[6], gt[3], Ht[6];
  double cost = huber_cost(Pb, ptb, J, N, mask, x, g, H);
  if (!(cost < __builtin_inf())) return;                 // NaN or inf
  double lambda = 1e-2;
  for (int trial = 0; trial < kRefineTrials; ++trial) {
    if (g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0) break;
    const double a = H[0] * (1.0 + lambda) + 1e-300, b = H[1], c = H[2];
    const double d = H[3] * (1.0 + lambda) + 1e-300, e = H[4], f = H[5] * (1.0 + lambda) + 1e-300;
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
    const double det = a * c00 + b * c01 + c * c02;
    const double di = -rcp_nr(det);
    double dx[3] = {di * (c00 * g[0] + c01 * g[1] + c02 * g[2]), di * (c01 * g[0] + c11 * g[1] + c12 * g[2]),
                    di * (c02 * g[0] + c12 * g[1] + c22 * g[2])};
    double xt[3] = {x[0] + dx[0], x[1] + dx[1], x[2] + dx[2]};
    const double ct = huber_cost(Pb, ptb, J, N, mask, xt, gt, Ht);
    const double d2 = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2];
    const double x2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (ct <= cost) {                                    // false for a NaN trial cost
      cost = ct;
#pragma unroll
      for (int i = 0; i < 3; ++i) { x[i] = xt[i]; g[i] = gt[i]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) H[i] = Ht[i];
      lambda = fmax(lambda * 0.2, 1e-12);
    } else {
      if (ct - cost <= 1e-14 * cost) break;              // not measurably worse: the cost has no more to say
      lambda *= 10.0;
      if (lambda > 1e12) break;
    }
    if (d2 <= 1e-18 * x2) break;                         // taken or not, a step this small ends it
  }
}

__global__ __launch_bounds__(kRansacBlock) void ransac_kernel(
    const float* __restrict__ P, const float* __restrict__ pts, const int32_t* __restrict__ pairs,
    int pairs_per_point, int n_iters, float epsilon, int direct_optimization, float* __restrict__ out_xyz,
    uint32_t* __restrict__ out_inliers, float* __restrict__ out_error_mean, int B, int N, int J) {
  const int n = B * J;
  const int h = threadIdx.x % kRansacGroup;
  const int slot = blockIdx.x * kRansacPoints + threadIdx.x / kRansacGroup;
  // a group past the end recomputes the last point and stores nothing: every lane of the
  // wave stays in the shuffles
  const bool live = slot < n;
  const int t = live ? slot : n - 1;
  const int b = t / J, j = t - b * J;
  const float* Pb = P + size_t(b) * N * 12;
  const float* ptb = pts + (size_t(b) * N * J + j) * 2;          // view v at ptb + v * J * 2
  const int32_t* pr = pairs + (pairs_per_point ? size_t(t) * n_iters * 2 : size_t(0));
  const double eps = double(epsilon);
  const uint32_t all_views = N >= 32 ? 0xffffffffu : ((1u << N) - 1u);

  // ---- hypotheses h, h + 16, ...: keep the first of the largest inlier count
  int best_count = 0, best_i = 0x7fffffff;
  uint32_t best_mask = 0u;
  for (int i = h; i < n_iters; i += kRansacGroup) {
    const int va = pr[size_t(i) * 2 + 0], vb = pr[size_t(i) * 2 + 1];
    if (va < 0 || va >= N || vb < 0 || vb >= N || va == vb) continue;
    double R[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) R[r][k] = 0.0;
    // the reference sorts the pair (triangulation.py:85)
    const int v0 = va < vb ? va : vb, v1 = va < vb ? vb : va;
    fold_view(R, Pb + size_t(v0) * 12, ptb[size_t(v0) * J * 2], ptb[size_t(v0) * J * 2 + 1]);
    fold_view(R, Pb + size_t(v1) * 12, ptb[size_t(v1) * J * 2], ptb[size_t(v1) * J * 2 + 1]);
    double x[3];
    solve_point(R, x);
    uint32_t mask = (1u << v0) | (1u << v1);
    for (int v = 0; v < N; ++v) {
      const float* pt = ptb + size_t(v) * J * 2;
      const double err = half_distance(project(Pb + size_t(v) * 12, pt[0], pt[1], x));
      if (err < eps) mask |= 1u << v;                    // false for a NaN error
    }
    const int count = __popc(mask);
    if (count > best_count) { best_count = count; best_i = i; best_mask = mask; }
  }
  // ---- (most inliers, lowest i) over the group's 16 lanes
#pragma unroll
  for (int o = kRansacGroup / 2; o > 0; o >>= 1) {
    const int oc = __shfl_xor(best_count, o, kRansacGroup);
    const int oi = __shfl_xor(best_i, o, kRansacGroup);
    const uint32_t om = uint32_t(__shfl_xor(int(best_mask), o, kRansacGroup));
    if (oc > best_count || (oc == best_count && oi < best_i)) { best_count = oc; best_i = oi; best_mask = om; }
  }
  const uint32_t mask = best_count > 0 ? best_mask : all_views;   // triangulation.py:100-101

  // ---- DLT over the inlier views (triangulation.py:103-107), then the refinement
  double R[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) R[r][k] = 0.0;
  for (int v = 0; v < N; ++v) {
    if (!((mask >> v) & 1u)) continue;
    fold_view(R, Pb + size_t(v) * 12, ptb[size_t(v) * J * 2], ptb[size_t(v) * J * 2 + 1]);
  }
  double x[3];
  solve_point(R, x);
  if (direct_optimization) refine(Pb, ptb, J, N, mask, x);

  // ---- mean reprojection error over the inlier views at the point as returned (f32)
  const float xf[3] = {float(x[0]), float(x[1]), float(x[2])};
  float mean = 0.f;
  if (out_error_mean) {
    const double xr[3] = {double(xf[0]), double(xf[1]), double(xf[2])};
    double sum = 0.0;
    for (int v = 0; v < N; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const float* pt = ptb + size_t(v) * J * 2;
      sum += half_distance(project(Pb + size_t(v) * 12, pt[0], pt[1], xr));
    }
    mean = float(sum / double(__popc(mask)));
  }
  if (live && h == 0) {
    float* o = out_xyz + size_t(t) * 3;
    o[0] = xf[0];
    o[1] = xf[1];
    o[2] = xf[2];
    out_inliers[t] = mask;
    if (out_error_mean) out_error_mean[t] = mean;
  }
}

constexpr int kReprojBlock = 256;

// One lane per (b, j, v): out[b][j][v] = |pts[b][v][j] - proj_v(X[b][j])| / 2, f64 arithmetic.
__global__ __launch_bounds__(kReprojBlock) void reprojection_error_kernel(
    const float* __restrict__ X, const float* __restrict__ pts, const float* __restrict__ P,
    float* __restrict__ out, int B, int N, int J) {
  const size_t t = size_t(blockIdx.x) * kReprojBlock + threadIdx.x;
  if (t >= size_t(B) * J * N) return;
  const int v = int(t % N);
  const size_t bj = t / N;
  const int j = int(bj % J), b = int(bj / J);
  const double x[3] = {double(X[bj * 3 + 0]), double(X[bj * 3 + 1]), double(X[bj * 3 + 2])};
  const float* pt = pts + ((size_t(b) * N + v) * J + j) * 2;
  out[t] = float(half_distance(project(P + (size_t(b) * N + v) * 12, pt[0], pt[1], x)));
}

}  // namespace
}  // namespace mvn

extern "C" int mvn_reprojection_error(const float* points3d, const float* pts, const float* proj, float* out,
                                      int B, int N, int J, void* stream) {
  using namespace mvn;
  if (!points3d || !pts || !proj || !out) return MVN_ERR_ARG;
  if (B <= 0 || N <= 0 || J <= 0) return MVN_ERR_SHAPE;
  if ((long long)B * J > (1LL << 30) || (long long)B * J * N > (1LL << 31) - 1) return MVN_ERR_SHAPE;
  const long long n = (long long)B * J * N;
  reprojection_error_kernel<<<unsigned((n + kReprojBlock - 1) / kReprojBlock), kReprojBlock, 0,
                              static_cast<hipStream_t>(stream)>>>(points3d, pts, proj, out, B, N, J);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" int mvn_triangulate_ransac(const float* proj, const float* pts, const int32_t* pairs, int pairs_per_point,
                                      int n_iters, float epsilon, int direct_optimization, float* out_xyz,
                                      uint32_t* out_inliers, float* out_error_mean, int B, int N, int J,
                                      void* stream) {
  using namespace mvn;
  if (!proj || !pts || !pairs || !out_xyz || !out_inliers) return MVN_ERR_ARG;
  if ((pairs_per_point != 0 && pairs_per_point != 1) || (direct_optimization != 0 && direct_optimization != 1))
    return MVN_ERR_ARG;
  if (B <= 0 || J <= 0 || N < 2 || N > kRansacMaxViews) return MVN_ERR_SHAPE;
  if (n_iters < 1 || n_iters > kRansacMaxIters) return MVN_ERR_SHAPE;
  if ((long long)B * J > (1LL << 30)) return MVN_ERR_SHAPE;
  const int n = B * J;
  ransac_kernel<<<(n + kRansacPoints - 1) / kRansacPoints, kRansacBlock, 0, static_cast<hipStream_t>(stream)>>>(
      proj, pts, pairs, pairs_per_point, n_iters, epsilon, direct_optimization, out_xyz, out_inliers, out_error_mean,
      B, N, J);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}
