// The two per-map bodies of the 2D soft-argmax, shared by softargmax2d.hip (one map per block)
// and algebraic.hip (one (b, j) per block, one map per 256-thread group and round): whoever
// calls them gets the same bits for (sum e*w / sum e, sum e*h / sum e) and the returned map.
//
// A body is run by kBlock threads, t in [0, kBlock) the caller's index within them, with
// `red` their own 3 x kWaves floats of LDS.  Its barriers are __syncthreads(): every thread of
// the block must call the same body the same number of times (1 barrier, 3 with SOFTMAX).
// `emit(x, y)` is called by t == 0 once the moments are reduced, before the map is written.
#pragma once

#include <math.h>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace mvn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

// Three passes over map `map` of hm (n = H * W pixels each, any shape and alignment): the max,
// then (sum e, sum e*w, sum e*h), then the normalised map into out (skipped when out is null).
template <typename T, typename TO, bool SOFTMAX, typename Emit>
__device__ __forceinline__ void softargmax2d_map(const T* hm, float mult, TO* out, size_t map,
                                                 int H, int W, int t, float (&red)[3][kWaves], Emit emit) {
  const int lane = t & (kWave - 1), wid = t / kWave;
  const int n = H * W;
  const T* p = hm + map * size_t(n);

  // pass 1: max of mult * x (softmax only)
  float M = 0.f;
  if constexpr (SOFTMAX) {
    float lm = -INFINITY;
    for (int i = t; i < n; i += kBlock) lm = fmaxf(lm, to_f32(p[i]) * mult);
    lm = wave_max63(lm);
    if (lane == kWave - 1) red[0][wid] = lm;
    __syncthreads();
    M = red[0][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) M = fmaxf(M, red[0][w]);
    __syncthreads();
  }

  // pass 2: mass and first moments
  float s = 0.f, sx = 0.f, sy = 0.f;
  for (int i = t; i < n; i += kBlock) {
    const float v = to_f32(p[i]) * mult;
    const float e = SOFTMAX ? __expf(v - M) : relu_keep_nan(v);
    const int h = i / W, w = i - h * W;
    s += e;
    sx = __builtin_fmaf(e, float(w), sx);
    sy = __builtin_fmaf(e, float(h), sy);
  }
  s = wave_sum63(s); sx = wave_sum63(sx); sy = wave_sum63(sy);
  if (lane == kWave - 1) { red[0][wid] = s; red[1][wid] = sx; red[2][wid] = sy; }
  __syncthreads();
  s = red[0][0]; sx = red[1][0]; sy = red[2][0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) { s += red[0][w]; sx += red[1][w]; sy += red[2][w]; }
  if (t == 0) emit(sx / s, sy / s);           // op.py:34, 40: x, y normalised by the mass

  // pass 3: the returned map — softmax normalised, relu as is (op.py:25-27)
  if (out != nullptr) {
    const float inv = 1.f / s;
    TO* o = out + map * size_t(n);
    for (int i = t; i < n; i += kBlock) {
      const float v = to_f32(p[i]) * mult;
      store_elem(o + i, SOFTMAX ? __expf(v - M) * inv : relu_keep_nan(v));
    }
  }
}

// Register-resident form (r17) for maps of at most kBlock * 4 * RUNS pixels with W % 4 == 0 and
// 16-byte aligned maps (every BASELINE config: 96^2): each thread loads its runs of 4
// consecutive pixels ONCE (vector loads), reduces the max, then (sum e, sum e*w, sum e*h), and
// writes the normalised map from registers — one pass over memory instead of three, and the
// (h, w) of a run from one division instead of one per pixel.  Config 1's 4 x 17 maps of 96^2:
// 16.6 -> 4.9 us (256 x 17 maps: 105 -> 64 us), profiles/r17_ab_softargmax2d.txt.
constexpr int kRuns = 12;                      // up to 12,288 pixels per map

// Whether the register form applies to maps of H x W read from hm and written to out (or not
// written: null) — one decision per launch, from the base pointers.
inline bool softargmax2d_reg_applies(const void* hm, const void* out, int H, int W) {
  return (long long)H * W <= (long long)kBlock * 4 * kRuns && W % 4 == 0 &&
         reinterpret_cast<uintptr_t>(hm) % 16 == 0 && (out == nullptr || reinterpret_cast<uintptr_t>(out) % 16 == 0);
}

template <typename T, typename TO, bool SOFTMAX, typename Emit>
__device__ __forceinline__ void softargmax2d_map_reg(const T* hm, float mult, TO* out,
                                                     size_t map, int H, int W, int t, float (&red)[3][kWaves],
                                                     Emit emit) {
  const int lane = t & (kWave - 1), wid = t / kWave;
  const int n = H * W;
  const T* p = hm + map * size_t(n);
  float v[kRuns][4];
#pragma unroll
  for (int r = 0; r < kRuns; ++r) {
    const int i = (r * kBlock + t) * 4;
    if (i < n) {
      if constexpr (sizeof(T) == 4) widen<T>(*reinterpret_cast<const u4v*>(p + i), v[r]);
      else widen(*reinterpret_cast<const u2v*>(p + i), v[r]);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[r][k] = v[r][k] * mult;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[r][k] = SOFTMAX ? -INFINITY : 0.f;
    }
  }
  float M = 0.f;
  if constexpr (SOFTMAX) {
    float lm = -INFINITY;
#pragma unroll
    for (int r = 0; r < kRuns; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) lm = fmaxf(lm, v[r][k]);
    lm = wave_max63(lm);
    if (lane == kWave - 1) red[0][wid] = lm;
    __syncthreads();
    M = red[0][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) M = fmaxf(M, red[0][w]);
    __syncthreads();
  }
  float s = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
  for (int r = 0; r < kRuns; ++r) {
    const int i = (r * kBlock + t) * 4;
    if (i >= n) continue;
    const int h = i / W, w0 = i - h * W;      // a run of 4 stays in one row (W % 4 == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float e = SOFTMAX ? __expf(v[r][k] - M) : relu_keep_nan(v[r][k]);
      v[r][k] = e;
      s += e;
      sx = __builtin_fmaf(e, float(w0 + k), sx);
      sy = __builtin_fmaf(e, float(h), sy);
    }
  }
  s = wave_sum63(s); sx = wave_sum63(sx); sy = wave_sum63(sy);
  if (lane == kWave - 1) { red[0][wid] = s; red[1][wid] = sx; red[2][wid] = sy; }
  __syncthreads();
  s = red[0][0]; sx = red[1][0]; sy = red[2][0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) { s += red[0][w]; sx += red[1][w]; sy += red[2][w]; }
  if (t == 0) emit(sx / s, sy / s);
  if (out != nullptr) {
    const float inv = SOFTMAX ? 1.f / s : 1.f;
    TO* o = out + map * size_t(n);
#pragma unroll
    for (int r = 0; r < kRuns; ++r) {
      const int i = (r * kBlock + t) * 4;
      if (i >= n) continue;
      float y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] = SOFTMAX ? v[r][k] * inv : v[r][k];
      if constexpr (sizeof(TO) == 4)
        *reinterpret_cast<float4*>(o + i) = make_float4(y[0], y[1], y[2], y[3]);
      else
        *reinterpret_cast<uint2*>(o + i) = make_uint2(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]));
    }
  }
}

}  // namespace
}  // namespace mvn
