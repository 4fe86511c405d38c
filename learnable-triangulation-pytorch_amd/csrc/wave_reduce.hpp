// Wave-level pieces shared by the soft-argmax kernels (softargmax.hip, softargmax2d.hpp and
// through it algebraic.hip, backward.hip): DPP reductions valid in lane 63, the online-softmax
// merge with its wave fold, and the widening of raw 16- / 8-byte loads to f32.
#pragma once

#include <math.h>

#include "common.hpp"

namespace mvn {

// ---- raw loads -> f32 ---------------------------------------------------------------------
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

// 16 raw bytes of T to 4 f32 or 8 bf16-as-f32 (exact: bits << 16), in element order.
template <typename T, int n>
__device__ __forceinline__ void widen(const u4v q, float (&v)[n]) {
  static_assert(n * sizeof(T) == 16, "one 16-byte run");
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (sizeof(T) == 4) {
      v[k] = __uint_as_float(q[k]);
    } else {
      v[2 * k] = __uint_as_float(q[k] << 16);
      v[2 * k + 1] = __uint_as_float(q[k] & 0xffff0000u);
    }
  }
}
// 8 raw bytes of bf16 to 4 f32.
__device__ __forceinline__ void widen(const u2v q, float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    v[2 * k] = __uint_as_float(q[k] << 16);
    v[2 * k + 1] = __uint_as_float(q[k] & 0xffff0000u);
  }
}

// ---- wave reductions valid in lane 63 -----------------------------------------------------
// row_shr DPP steps, then row_bcast:15 / row_bcast:31 (6 DPP-fused VALU ops each).
template <int CTRL, int RMASK> __device__ __forceinline__ float dpp_f(float v, float ident) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ident), __float_as_int(v), CTRL, RMASK, 0xf, false));
}
// (the max written as DPP-fused v_max_f32 with dst == src1: a lane without a source is
// disabled and keeps its value; through fmaxf every DPP result was canonicalised first.
// v_max_f32 returns the other operand for a quiet NaN, as fmaxf does.)
__device__ __forceinline__ float wave_max63(float v) {
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(v));
  return v;
}
__device__ __forceinline__ float wave_sum63(float v) {
  v += dpp_f<0x111, 0xf>(v, 0.f); v += dpp_f<0x112, 0xf>(v, 0.f);
  v += dpp_f<0x114, 0xf>(v, 0.f); v += dpp_f<0x118, 0xf>(v, 0.f);
  v += dpp_f<0x142, 0xa>(v, 0.f); v += dpp_f<0x143, 0xc>(v, 0.f);
  return v;
}
// Lane 63's value, wave-uniform.
__device__ __forceinline__ float lane63(float v) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), kWave - 1));
}

// ---- online-softmax merge -----------------------------------------------------------------
// Fold (m2, s2) into (m, s): N running sums of exponentials taken against the running max m,
// rescaled to the common max.  A side whose max is -inf holds no mass and gets factor 0
// (exp(-inf - -inf) would be NaN).  Without SOFTMAX (relu) the sums simply add and m is unused.
template <bool SOFTMAX, int N>
__device__ __forceinline__ void softmax_merge(float& m, float (&s)[N], float m2, const float (&s2)[N]) {
  if constexpr (SOFTMAX) {
    const float M = fmaxf(m, m2);
    const float ka = (m == -INFINITY) ? 0.f : __expf(m - M);
    const float kb = (m2 == -INFINITY) ? 0.f : __expf(m2 - M);
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = s[i] * ka + s2[i] * kb;
    m = M;
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += s2[i];
  }
}
// The wave's 64 (m, s) folded by xor butterflies: every lane ends with the result.
template <bool SOFTMAX, int N>
__device__ __forceinline__ void wave_softmax_merge(float& m, float (&s)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, kWave);
    float s2[N];
#pragma unroll
    for (int i = 0; i < N; ++i) s2[i] = __shfl_xor(s[i], o, kWave);
    softmax_merge<SOFTMAX>(m, s, m2, s2);
  }
}

}  // namespace mvn
