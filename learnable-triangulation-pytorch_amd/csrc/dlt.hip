// Batched confidence-weighted algebraic (DLT) triangulation for gfx950.
//
// Replaces mvn/utils/multiview.py:162-174 (triangulate_batch_of_points) and its
// per-point solver multiview.py:132-159.  The reference loops over B x J in Python
// and calls torch.svd on each 2N x 4 matrix (B*J LAPACK / rocSOLVER calls).
//
// Here one lane owns one (b, j):
//   1. rows of A are formed in f32 exactly as multiview.py:150-152 forms them
//      (A = P[2]*pt; A -= P[:2]; A *= conf — three separately rounded ops),
//   2. each row is folded into a 4x4 upper-triangular R by Givens rotations (f64,
//      Newton-refined hardware reciprocal square roots: round 3, config 1 latency),
//      so R^T R = A^T A without ever squaring the condition number and for any N,
//   3. the right singular vector of the smallest singular value is the homogeneous point
//      (multiview.py:154-156): inverse iteration on R^T R (4-6 steps), or, when that does
//      not converge (near-equal smallest singular values) or settles on another singular
//      vector (a null vector orthogonal to its start), a one-sided Jacobi SVD of R (f64),
//   4. X[:3] / X[3] (multiview.py:157; sign of the null vector cancels).
#include "common.hpp"
#include "dlt_solver.hpp"

namespace mvn {
namespace {

constexpr int kDltBlock = 64;

__global__ __launch_bounds__(kDltBlock) void dlt_kernel(const float* __restrict__ P, const float* __restrict__ pts,
                                                        const float* __restrict__ conf, float* __restrict__ out,
                                                        int B, int N, int J) {
  const int t = blockIdx.x * kDltBlock + threadIdx.x;
  if (t >= B * J) return;
  const int b = t / J, j = t - b * J;

  float x[3];
  dlt_point(P, pts, conf, b, j, N, J, x);
  float* o = out + size_t(t) * 3;
  o[0] = x[0];
  o[1] = x[1];
  o[2] = x[2];
}

// dlt_kernel with the solver's trace parameter on (mvn_debug_dlt_trace): the same dlt_point, so
// the same bits in out, plus the path taken and its step count per point.
__global__ __launch_bounds__(kDltBlock) void dlt_trace_kernel(const float* __restrict__ P, const float* __restrict__ pts,
                                                              const float* __restrict__ conf, float* __restrict__ out,
                                                              int* __restrict__ path, int* __restrict__ steps, int B,
                                                              int N, int J) {
  const int t = blockIdx.x * kDltBlock + threadIdx.x;
  if (t >= B * J) return;
  const int b = t / J, j = t - b * J;

  float x[3];
  int pa = 0, st = 0;
  dlt_point<true>(P, pts, conf, b, j, N, J, x, &pa, &st);
  float* o = out + size_t(t) * 3;
  o[0] = x[0];
  o[1] = x[1];
  o[2] = x[2];
  path[t] = pa;
  steps[t] = st;
}

}  // namespace
}  // namespace mvn

extern "C" int mvn_dlt(const float* proj, const float* pts, const float* conf, float* out, int B, int N, int J,
                       void* stream) {
  using namespace mvn;
  if (!proj || !pts || !out) return MVN_ERR_ARG;
  if (B <= 0 || N <= 0 || J <= 0) return MVN_ERR_SHAPE;
  if ((long long)B * J > (1LL << 30)) return MVN_ERR_SHAPE;
  const int n = B * J;
  dlt_kernel<<<(n + kDltBlock - 1) / kDltBlock, kDltBlock, 0, static_cast<hipStream_t>(stream)>>>(proj, pts, conf, out, B, N, J);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" int mvn_debug_dlt_trace(const float* proj, const float* pts, const float* conf, float* out_xyz, int* path,
                                   int* steps, int B, int N, int J, void* stream) {
  using namespace mvn;
  if (!proj || !pts || !out_xyz || !path || !steps) return MVN_ERR_ARG;
  if (B <= 0 || N <= 0 || J <= 0) return MVN_ERR_SHAPE;
  if ((long long)B * J > (1LL << 30)) return MVN_ERR_SHAPE;
  const int n = B * J;
  dlt_trace_kernel<<<(n + kDltBlock - 1) / kDltBlock, kDltBlock, 0, static_cast<hipStream_t>(stream)>>>(
      proj, pts, conf, out_xyz, path, steps, B, N, J);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" int mvn_version(void) { return (0 << 16) | (1 << 8) | 0; }

extern "C" const char* mvn_strerror(int code) {
  switch (code) {
    case MVN_OK: return "ok";
    case MVN_ERR_ARG: return "invalid argument (null pointer, enum or flag)";
    case MVN_ERR_SHAPE: return "invalid shape (non-positive or too large extent)";
    case MVN_ERR_DTYPE: return "unsupported dtype combination";
    case MVN_ERR_LAUNCH: return "HIP kernel launch failed";
    case MVN_ERR_WORKSPACE: return "workspace missing or too small";
  }
  return "unknown error";
}
