// The algebraic model's forward in one launch, for gfx950: heatmaps -> 2D soft-argmax per
// view -> confidence normalisation -> upscale to image pixels -> confidence-weighted DLT.
//
// Replaces the chain of mvn/models/triangulation.py:164-191 (AlgebraicTriangulationNet.forward
// after the backbone), which the separate kernels run as mvn_softargmax2d, six torch
// elementwise / reduce launches and mvn_dlt: at batch 1 (4 views x 17 joints) the chain is
// launch-bound.
//
// One block per (b, j), 256 x VG threads: VG in {1, 2, 4} view groups of four waves.
//   1. views are taken in rounds of VG: group g runs the body of softargmax2d.hpp (the same
//      device functions as mvn_softargmax2d's kernels: same bits) on view g, g + VG, ...;
//      thread 0 of the group writes the view's (x, y) to out_xy, and the upscaled point
//      (x * scale_x, y * scale_y) to out_kp2d and to LDS.  A group without a view in the
//      last round (N = 3 with VG = 4; N = 5) runs the body on the last view again and writes
//      nothing: the bodies' barriers are block-wide.
//   2. one barrier after every round (the next round reuses the reduction words; after the
//      last one the points are visible), then every wave but wave 0 returns.
//   3. wave 0, all lanes redundantly (no divergence; lane 0 stores): s = sum_v conf[b, v, j] as
//      a sequential f32 sum in view order, c_v = conf_v / s + 1e-5f (triangulation.py:173-174,
//      IEEE division), then dlt_point (dlt_solver.hpp, the function dlt_kernel runs: same bits)
//      on the upscaled points and the c_v, both read from LDS.
#include "common.hpp"
#include "dlt_solver.hpp"
#include "softargmax2d.hpp"

namespace mvn {
namespace {

constexpr int kAlgMaxViews = 32;               // LDS holds the views' points and confidences

template <typename T, typename TO, bool SOFTMAX, int VG>
__global__ __launch_bounds__(kBlock * VG) void algebraic_kernel(
    const T* __restrict__ hm, float mult, const float* __restrict__ P, const float* __restrict__ conf, float scale_x,
    float scale_y, float* __restrict__ out_xyz, float* __restrict__ out_kp2d, float* __restrict__ out_xy,
    float* __restrict__ out_conf, TO* __restrict__ out_maps, int reg, int N, int J, int H, int W) {
  __shared__ float red[VG][3][kWaves];
  __shared__ float s_pt[kAlgMaxViews][2];       // image pixels
  __shared__ float s_c[kAlgMaxViews];           // normalised confidences
  const int g = threadIdx.x / kBlock, t = threadIdx.x % kBlock;
  const int b = blockIdx.x / J, j = blockIdx.x - b * J;

  for (int v0 = 0; v0 < N; v0 += VG) {
    const bool live = v0 + g < N;
    const int v = live ? v0 + g : N - 1;
    const size_t map = (size_t(b) * N + v) * J + j;
    TO* o = live ? out_maps : nullptr;
    int Hr = H, Wr = W;
    // 1024 threads leave a lane 128 registers: keep the compiler from hoisting every run's
    // (h, w) out of the rounds loop (two dozen live values, spilled), at no cost for N <= 4
    if constexpr (VG == 4) asm volatile("" : "+s"(Hr), "+s"(Wr));
    auto emit = [&](float x, float y) {
      if (!live) return;
      MVN_DASSERT(v >= 0 && v < kAlgMaxViews);
      const float px = x * scale_x, py = y * scale_y;      // triangulation.py:182-183
      s_pt[v][0] = px;
      s_pt[v][1] = py;
      out_xy[map * 2] = x;
      out_xy[map * 2 + 1] = y;
      out_kp2d[map * 2] = px;
      out_kp2d[map * 2 + 1] = py;
    };
    if (reg) softargmax2d_map_reg<T, TO, SOFTMAX>(hm, mult, o, map, Hr, Wr, t, red[g], emit);
    else softargmax2d_map<T, TO, SOFTMAX>(hm, mult, o, map, Hr, Wr, t, red[g], emit);
    __syncthreads();
  }
  if (threadIdx.x >= kWave) return;

  // ---- wave 0: confidences (triangulation.py:161, 173-174), then the DLT
  const size_t cj = size_t(b) * N * J + j;       // view v at cj + v * J
  float s = 0.f;
  for (int v = 0; v < N; ++v) {
    const float c = conf ? conf[cj + size_t(v) * J] : 1.f;
    s = v == 0 ? c : s + c;
  }
  for (int v = 0; v < N; ++v) {
    const float c = conf ? conf[cj + size_t(v) * J] : 1.f;
    const float cn = c / s + 1e-5f;
    MVN_DASSERT(v >= 0 && v < kAlgMaxViews);
    s_c[v] = cn;
    if (t == 0) out_conf[cj + size_t(v) * J] = cn;
  }
  float x[3];
  // A batch index the compiler must take for lane-variant (it is 0): with inputs it knows to
  // be wave-uniform it branches instead of predicating, and that form of the Jacobi fallback
  // needs 133 registers where dlt_kernel's needs 124 — over the 128 of a 1024-thread block.
  int z = 0;
  asm volatile("" : "+v"(z));
  dlt_point(P + size_t(b) * N * 12, &s_pt[0][0], s_c, z, 0, N, 1, x);     // this point's views as a (1, N, 1) batch
  if (t == 0) {
    // three dword stores, not one of 12 bytes: the store-hazard scan (tools/check_store_hazard.py)
    // reads on past the s_endpgm that follows into the next block's first VALU write
    volatile float* o = out_xyz + size_t(blockIdx.x) * 3;
    o[0] = x[0];
    o[1] = x[1];
    o[2] = x[2];
  }
}

template <typename T, typename TO, bool SOFTMAX, int VG, typename... A>
void launch_vg(int blocks, hipStream_t s, A... a) {
  algebraic_kernel<T, TO, SOFTMAX, VG><<<blocks, kBlock * VG, 0, s>>>(a...);
}

template <typename T, typename TO>
int launch(const void* hm, float mult, int softmax, const float* P, const float* conf, float sx, float sy, float* xyz,
           float* kp2d, float* xy, float* cn, void* maps, int B, int N, int J, int H, int W, hipStream_t s) {
  const int reg = softargmax2d_reg_applies(hm, maps, H, W) ? 1 : 0;
  const int vg = N >= 3 ? 4 : N;                // the smallest of {1, 2, 4} covering min(N, 4)
  const T* h = static_cast<const T*>(hm);
  TO* m = static_cast<TO*>(maps);
  const int blocks = B * J;
#define MVN_ALG_LAUNCH(SM, VG) launch_vg<T, TO, SM, VG>(blocks, s, h, mult, P, conf, sx, sy, xyz, kp2d, xy, cn, m, reg, N, J, H, W)
  if (softmax) {
    if (vg == 1) MVN_ALG_LAUNCH(true, 1); else if (vg == 2) MVN_ALG_LAUNCH(true, 2); else MVN_ALG_LAUNCH(true, 4);
  } else {
    if (vg == 1) MVN_ALG_LAUNCH(false, 1); else if (vg == 2) MVN_ALG_LAUNCH(false, 2); else MVN_ALG_LAUNCH(false, 4);
  }
#undef MVN_ALG_LAUNCH
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

}  // namespace
}  // namespace mvn

extern "C" int mvn_algebraic_triangulate(const void* heatmaps, int dtype, float multiplier, int softmax,
                                         const float* proj, const float* conf, float scale_x, float scale_y,
                                         float* out_xyz, float* out_kp2d, float* out_xy, float* out_conf,
                                         void* out_maps, int maps_dtype, int B, int N, int J, int H, int W,
                                         void* stream) {
  using namespace mvn;
  if (!heatmaps || !proj || !out_xyz || !out_kp2d || !out_xy || !out_conf) return MVN_ERR_ARG;
  if (softmax != 0 && softmax != 1) return MVN_ERR_ARG;
  if (B <= 0 || N <= 0 || J <= 0 || H <= 0 || W <= 0 || N > kAlgMaxViews) return MVN_ERR_SHAPE;
  if ((long long)B * J > (1LL << 30) || (long long)B * N * J > (1LL << 31) - 1 || (long long)H * W > (1LL << 30))
    return MVN_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == MVN_DTYPE_F32 && maps_dtype == MVN_DTYPE_F32)
    return launch<float, float>(heatmaps, multiplier, softmax, proj, conf, scale_x, scale_y, out_xyz, out_kp2d, out_xy,
                                out_conf, out_maps, B, N, J, H, W, s);
  if (dtype == MVN_DTYPE_BF16 && maps_dtype == MVN_DTYPE_BF16)
    return launch<uint16_t, uint16_t>(heatmaps, multiplier, softmax, proj, conf, scale_x, scale_y, out_xyz, out_kp2d,
                                      out_xy, out_conf, out_maps, B, N, J, H, W, s);
  if (dtype == MVN_DTYPE_BF16 && maps_dtype == MVN_DTYPE_F32)
    return launch<uint16_t, float>(heatmaps, multiplier, softmax, proj, conf, scale_x, scale_y, out_xyz, out_kp2d,
                                   out_xy, out_conf, out_maps, B, N, J, H, W, s);
  return MVN_ERR_DTYPE;
}
