// The f64 null-vector solver shared by the DLT kernels (dlt.hip, ransac.hip): Newton-refined
// reciprocals, the streaming Givens fold of rows into a 4x4 upper-triangular R, inverse
// iteration on R^T R, the inertia check of what it converged to, and the one-sided Jacobi SVD
// it falls back to (null_vector ties the three together).
#pragma once

#include "common.hpp"

namespace mvn {
namespace {

// f64 reciprocal and reciprocal square root: the hardware estimates (v_rcp_f64 / v_rsq_f64,
// about half the mantissa) refined by two Newton steps (fma): within an ulp or two of the IEEE
// result, in ~5 dependent operations instead of the ~10-20 of IEEE '/', sqrt and hypot.  The
// solve is one lane's serial f64 chain, so its latency is the kernel's time (config 1).
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
  return __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double h = 0.5 * y, g = x * y;
    y = __builtin_fma(y, __builtin_fma(-g, h, 0.5), y);   // y (1.5 - x y^2 / 2)
  }
  return y;
}

// Fold row a into the upper-triangular R: one Givens rotation per non-zero entry
// (r = |(R_kk, a_k)|, c = R_kk / r, s = a_k / r from one reciprocal square root).
__device__ __forceinline__ void givens_fold(double (&R)[4][4], double (&a)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (a[k] == 0.0) continue;
    const double n2 = __builtin_fma(R[k][k], R[k][k], a[k] * a[k]);
    const double ri = rsqrt_nr(n2);
    const double c = R[k][k] * ri, s = a[k] * ri;
    R[k][k] = n2 * ri;
    a[k] = 0.0;
#pragma unroll
    for (int l = k + 1; l < 4; ++l) {
      const double rk = R[k][l], al = a[l];
      R[k][l] = c * rk + s * al;
      a[l] = -s * rk + c * al;
    }
  }
}

// One-sided Jacobi on the columns of U (= R on entry); V accumulates the rotations.
// Convergence test |gamma| <= 1e-15 sqrt(alpha beta) as gamma^2 <= 1e-30 alpha beta (no sqrt).
// kTrace (mvn_debug_dlt_trace only): *sweeps = the sweeps run, the last, rotation-free one included.
template <bool kTrace = false>
__device__ __forceinline__ void jacobi_svd(double (&U)[4][4], double (&V)[4][4], int* sweeps = nullptr) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) V[i][k] = i == k ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    if (kTrace) *sweeps = sweep + 1;
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          alpha += U[i][p] * U[i][p];
          beta += U[i][q] * U[i][q];
          gamma += U[i][p] * U[i][q];
        }
        if (gamma == 0.0 || gamma * gamma <= 1e-30 * (alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) * rcp_nr(2.0 * gamma);
        const double z2 = __builtin_fma(zeta, zeta, 1.0);
        const double root = z2 * rsqrt_nr(z2);                       // sqrt(1 + zeta^2)
        // |zeta| > 1e150: zeta^2 overflows (inf * rsqrt(inf) = NaN); there t = 1 / (2 zeta) to
        // working precision, which is what the IEEE form tends to.  A guard, not a path a test can
        // take: with the convergence test above it needs alpha < 2.5e-271 beta, and columns that
        // come from f32 rows are exactly zero (gamma == 0: skipped) or span at most 1e-168 in
        // alpha / beta on entry and sink no further than rounding level, ~1e-32 beta, under the
        // rotations
        const double t = fabs(zeta) > 1e150 ? 0.5 * rcp_nr(zeta)
                                            : (zeta >= 0.0 ? 1.0 : -1.0) * rcp_nr(fabs(zeta) + root);
        const double c = rsqrt_nr(__builtin_fma(t, t, 1.0)), s = c * t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double up = U[i][p], uq = U[i][q];
          U[i][p] = c * up - s * uq;
          U[i][q] = s * up + c * uq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq;
          V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

// Null vector by inverse iteration on R^T R = A^T A (its eigenvector of the smallest eigenvalue,
// the right singular vector multiview.py:154-156 takes): two triangular solves per step, each
// vector rescaled by its largest entry and the result normalised.  The null component grows by
// (sigma_2 / sigma_min)^2 per step: at the bench and test geometries 4-6 steps reach a step
// change below 1e-10 (results within 2e-13 of the f64 LAPACK restatement, numpy model); still
// moving after 12 steps (near-equal smallest singular values) returns false and the caller
// runs the Jacobi SVD instead.  A zero
// pivot (an exact null vector) is replaced by 1e-30 of the largest one.
// kTrace (mvn_debug_dlt_trace only): *steps = the steps run.
template <bool kTrace = false>
__device__ __forceinline__ bool inverse_iteration(const double (&R)[4][4], double (&x)[4], int* steps = nullptr) {
  double dmax = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) dmax = fmax(dmax, fabs(R[k][k]));
  if (!(dmax > 0.0)) return false;
  double rinv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = R[k][k];
    rinv[k] = rcp_nr(fabs(d) > 1e-30 * dmax ? d : (d < 0.0 ? -1e-30 : 1e-30) * dmax);
  }
  auto rescale = [](double (&v)[4]) {
    const double m = fmax(fmax(fabs(v[0]), fabs(v[1])), fmax(fabs(v[2]), fabs(v[3])));
    const double r = rcp_nr(m);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] *= r;
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = 0.5;
  for (int it = 0; it < 12; ++it) {
    if (kTrace) *steps = it + 1;
    double z[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                 // R^T z = x (forward substitution)
      double acc = x[k];
#pragma unroll
      for (int i = 0; i < k; ++i) acc = __builtin_fma(-R[i][k], z[i], acc);
      z[k] = acc * rinv[k];
    }
    rescale(z);
#pragma unroll
    for (int k = 3; k >= 0; --k) {                // R y = z (back substitution)
      double acc = z[k];
#pragma unroll
      for (int l = k + 1; l < 4; ++l) acc = __builtin_fma(-R[k][l], y[l], acc);
      y[k] = acc * rinv[k];
    }
    rescale(y);
    const double n = rsqrt_nr(y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3]);
    const double sg = (y[0] * x[0] + y[1] * x[1] + y[2] * x[2] + y[3] * x[3]) < 0.0 ? -n : n;
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[i] *= sg;
      d += (y[i] - x[i]) * (y[i] - x[i]);
      x[i] = y[i];
    }
    if (!(d == d)) return false;                  // NaN (non-finite input): the Jacobi path decides
    if (it > 0 && d < 1e-20) return true;
  }
  return false;
}

// Is x, an eigenvector of R^T R that inverse iteration settled on, the one of the smallest
// eigenvalue?  The iteration starts from (1/2, 1/2, 1/2, 1/2); a null vector exactly orthogonal to
// that start, on data exact enough that no rounding error supplies the missing component, never
// enters, and the iteration stands still on another eigenvector and reports convergence (A =
// H diag(8, 4, 2, 1) H, H the 4x4 Hadamard matrix: the start is the eigenvector of 8).  Sylvester's
// law of inertia decides: R^T R - mu I has four positive LDL^T pivots exactly when no eigenvalue
// lies below mu.  mu = |R x|^2 - 1e-12 tr(R^T R): the Rayleigh quotient of a converged x is within
// ~1e-20 tr of its eigenvalue and the pivots' rounding error is ~1e-16 tr, so a right x always
// passes (and is returned untouched), and a wrong one fails unless the eigenvalue it missed lies
// within 1e-12 tr below its own (singular values that differ by less than 1e-6 |A|_F).  Ten
// products, three Newton reciprocals; NaN or a zero pivot compares false.
__device__ __forceinline__ bool is_smallest_eigenvector(const double (&R)[4][4], const double (&x)[4]) {
  double S[4][4];                                  // lower triangle of R^T R
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k <= i; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r <= k; ++r) acc = __builtin_fma(R[r][i], R[r][k], acc);
      S[i][k] = acc;
    }
  double lam = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double acc = 0.0;
#pragma unroll
    for (int k = r; k < 4; ++k) acc = __builtin_fma(R[r][k], x[k], acc);
    lam = __builtin_fma(acc, acc, lam);
  }
  const double mu = __builtin_fma(-1e-12, (S[0][0] + S[1][1]) + (S[2][2] + S[3][3]), lam);
#pragma unroll
  for (int i = 0; i < 4; ++i) S[i][i] -= mu;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                    // right-looking LDL^T, no pivoting
    ok &= S[k][k] > 0.0;
    if (k == 3) break;
    const double di = rcp_nr(S[k][k]);
#pragma unroll
    for (int i = k + 1; i < 4; ++i) {
      const double l = S[i][k] * di;
#pragma unroll
      for (int m = k + 1; m <= i; ++m) S[i][m] = __builtin_fma(-l, S[m][k], S[i][m]);
    }
  }
  return ok;
}

// The null vector X of the folded R, as every DLT kernel takes it (dlt_point below, ransac.hip).
// kTrace (mvn_debug_dlt_trace only): *path = 0 zero column, 1 inverse iteration, 2 Jacobi SVD;
// *steps = the inverse-iteration steps of path 1, the Jacobi sweeps of path 2, 0 on path 0.
template <bool kTrace = false>
__device__ __forceinline__ void null_vector(double (&R)[4][4], double (&X)[4], int* path = nullptr,
                                            int* steps = nullptr) {
  // An exactly zero column k of A (all-zero confidences, a coordinate no camera sees) leaves
  // R's column k exactly zero (the rotations mix rows, never columns), and e_k is an exact null
  // vector; LAPACK's SVD returns it as V[:, 3], the last of the tied smallest singular values
  // when there are several (A = 0: V = I, so e_4 and the point (0, 0, 0)).  The reference's
  // X[:3] / X[3] then gives (0, 0, 0) for k = 3 and (nan, nan, +-inf) otherwise
  // (multiview.py:154-157); iterating on the singular R would return ratios of tiny numbers.
  int zcol = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bool z = true;
#pragma unroll
    for (int i = 0; i <= k; ++i) z &= R[i][k] == 0.0;
    if (z) zcol = k;
  }
  if (kTrace) { *path = 0; *steps = 0; }
  if (zcol >= 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) X[i] = i == zcol ? 1.0 : 0.0;
  } else if (!(inverse_iteration<kTrace>(R, X, steps) && is_smallest_eigenvector(R, X))) {
    if (kTrace) *path = 2;
    double V[4][4];
    jacobi_svd<kTrace>(R, V, steps);
    int kmin = 0;
    double smin = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double n2 = R[0][k] * R[0][k] + R[1][k] * R[1][k] + R[2][k] * R[2][k] + R[3][k] * R[3][k];
      if (k == 0 || n2 <= smin) { smin = n2; kmin = k; }     // ties: the last, as LAPACK's order
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      X[i] = V[i][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) if (kmin == k) X[i] = V[i][k];
    }
  } else if (kTrace) {
    *path = 1;
  }
}

// One confidence-weighted DLT point (multiview.py:132-159), point (b, j) of P (B, N, 3, 4),
// pts (B, N, J, 2) and conf (B, N, J) or null (all ones).  Shared by dlt_kernel (dlt.hip: one
// lane per point, inputs in global memory) and algebraic_kernel (algebraic.hip: one point's
// pts and conf in LDS, as a (1, N, 1) batch), so both return the same bits.
//   1. rows of A in f32 exactly as multiview.py:150-152 forms them (A = P[2]*pt; A -= P[:2];
//      A *= conf — three separately rounded ops), folded into R by Givens rotations (f64),
//   2. the null vector (null_vector above): exact zero column, inverse iteration, or the Jacobi SVD,
//   3. X[:3] / X[3] (multiview.py:157; the sign of the null vector cancels).
template <bool kTrace = false>
__device__ __forceinline__ void dlt_point(const float* P, const float* pts, const float* conf, int b, int j, int N,
                                          int J, float (&o)[3], int* path = nullptr, int* steps = nullptr) {
  double R[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) R[i][k] = 0.0;

  for (int v = 0; v < N; ++v) {
    const float* Pv = P + (size_t(b) * N + v) * 12;
    const size_t pj = (size_t(b) * N + v) * J + j;
    const float pt[2] = {pts[pj * 2 + 0], pts[pj * 2 + 1]};
    const float cf = conf ? conf[pj] : 1.f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      double a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float e = Pv[8 + k] * pt[r];   // multiview.py:150
        e = e - Pv[r * 4 + k];         // multiview.py:151
        e = e * cf;                    // multiview.py:152
        a[k] = double(e);
      }
      givens_fold(R, a);
    }
  }

  double X[4];
  null_vector<kTrace>(R, X, path, steps);
  o[0] = float(X[0] / X[3]);
  o[1] = float(X[1] / X[3]);
  o[2] = float(X[2] / X[3]);
}

}  // namespace
}  // namespace mvn
