// 2D soft-argmax of per-view heatmaps for gfx950 — the algebraic path's producer of the
// DLT's 2D points.
//
// Replaces mvn/utils/op.py:11-47 (integrate_tensor_2d), with the caller's
// `heatmaps * heatmap_multiplier` (triangulation.py:164) fused:
//   softmax (op.py:25) or relu (op.py:27) over the flattened H*W map of every (b, j);
//   x = sum_w w * sum_h p[h, w], y = sum_h h * sum_w p[h, w] (op.py:31-38); with relu the
//   sums are divided by the mass (op.py:40-42), with softmax the map is already
//   normalised, so both modes are x = sum(p * w) / sum(p) — the exp / relu weights are
//   never normalised in registers, only the returned map is.
//
// One 256-thread block per map (a 96x96 map is 37 KB: three passes over it run from L2):
// pass 1 the max, pass 2 (sum e, sum e*w, sum e*h), pass 3 the normalised map (skipped when
// the caller does not want it).  Reductions: DPP within a wave, LDS across the 4 waves.
#include "common.hpp"
#include "softargmax2d.hpp"

namespace mvn {
namespace {

// The bodies are in softargmax2d.hpp (shared with algebraic.hip): here one map per block.
template <typename T, typename TO, bool SOFTMAX>
__global__ __launch_bounds__(kBlock) void softargmax2d(const T* __restrict__ hm, float mult, float* __restrict__ xy,
                                                      TO* __restrict__ out, int H, int W) {
  __shared__ float red[3][kWaves];
  const size_t map = blockIdx.x;
  softargmax2d_map<T, TO, SOFTMAX>(hm, mult, out, map, H, W, threadIdx.x, red, [&](float x, float y) {
    xy[map * 2] = x;
    xy[map * 2 + 1] = y;
  });
}

template <typename T, typename TO, bool SOFTMAX>
__global__ __launch_bounds__(kBlock) void softargmax2d_reg(const T* __restrict__ hm, float mult, float* __restrict__ xy,
                                                          TO* __restrict__ out, int H, int W) {
  __shared__ float red[3][kWaves];
  const size_t map = blockIdx.x;
  softargmax2d_map_reg<T, TO, SOFTMAX>(hm, mult, out, map, H, W, threadIdx.x, red, [&](float x, float y) {
    xy[map * 2] = x;
    xy[map * 2 + 1] = y;
  });
}

template <typename T, typename TO>
int launch(const void* hm, float mult, int softmax, float* xy, void* out, int maps, int H, int W, hipStream_t s) {
  if (softargmax2d_reg_applies(hm, out, H, W)) {
    if (softmax)
      softargmax2d_reg<T, TO, true><<<maps, kBlock, 0, s>>>(static_cast<const T*>(hm), mult, xy, static_cast<TO*>(out), H, W);
    else
      softargmax2d_reg<T, TO, false><<<maps, kBlock, 0, s>>>(static_cast<const T*>(hm), mult, xy, static_cast<TO*>(out), H, W);
    return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
  }
  if (softmax)
    softargmax2d<T, TO, true><<<maps, kBlock, 0, s>>>(static_cast<const T*>(hm), mult, xy, static_cast<TO*>(out), H, W);
  else
    softargmax2d<T, TO, false><<<maps, kBlock, 0, s>>>(static_cast<const T*>(hm), mult, xy, static_cast<TO*>(out), H, W);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

}  // namespace
}  // namespace mvn

extern "C" int mvn_softargmax2d(const void* heatmaps, int dtype, float multiplier, int softmax, float* out_xy,
                                void* out_maps, int out_dtype, int B, int J, int H, int W, void* stream) {
  using namespace mvn;
  if (!heatmaps || !out_xy) return MVN_ERR_ARG;
  if (softmax != 0 && softmax != 1) return MVN_ERR_ARG;
  if (B <= 0 || J <= 0 || H <= 0 || W <= 0) return MVN_ERR_SHAPE;
  if ((long long)B * J > (1LL << 31) - 1 || (long long)H * W > (1LL << 30)) return MVN_ERR_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int maps = B * J;
  if (dtype == MVN_DTYPE_F32 && out_dtype == MVN_DTYPE_F32)
    return launch<float, float>(heatmaps, multiplier, softmax, out_xy, out_maps, maps, H, W, s);
  if (dtype == MVN_DTYPE_BF16 && out_dtype == MVN_DTYPE_BF16)
    return launch<uint16_t, uint16_t>(heatmaps, multiplier, softmax, out_xy, out_maps, maps, H, W, s);
  if (dtype == MVN_DTYPE_BF16 && out_dtype == MVN_DTYPE_F32)
    return launch<uint16_t, float>(heatmaps, multiplier, softmax, out_xy, out_maps, maps, H, W, s);
  return MVN_ERR_DTYPE;
}
