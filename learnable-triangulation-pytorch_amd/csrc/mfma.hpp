// What the bf16 MFMA kernels of the V2V share (v2v_front, v2v_head, v2v_res3d, v2v_interior,
// v2v_deep): the operand types and the MFMA wrapper, the buffer resource of the range-checked
// loads (also the unprojection's, unproject_common.hpp), the convolutions' and upsamples' epilogue,
// and the host side's skip-argument checks and skip_mode dispatch.  Everything on the device is
// __forceinline__: each kernel's code is what it was with these written out in place.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace mvn {

constexpr uint32_t kOob = 0x80000000u;            // buffer byte offset past any frame: the load returns zero

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x32_bf16: a = 16 rows x 32 K-slots, b = 32 K-slots x 16 columns, each lane's
// 8 bf16 in 16 bytes (uint4, or v2v_head's Frag).
template <typename TB>
__device__ __forceinline__ f32x4_t mfma(const uint4& a, const TB& b, f32x4_t c) {
  static_assert(sizeof(TB) == 16, "an MFMA operand is 8 bf16");
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                 0, 0, 0);
}

// Buffer descriptor from block-uniform inputs, provably in SGPRs (cdna_hip_programming.md T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(a));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(a >> 32));
  void* p = reinterpret_cast<void*>((uint64_t(hi) << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(p, 0, int(__builtin_amdgcn_readfirstlane(bytes)), 0x00020000);
}

// bf16 i (0..3) of four consecutive channels loaded as 8 bytes, widened to f32.
__device__ __forceinline__ float bf16_of_pair(const uint2& q, int i) {
  const uint32_t pair = i < 2 ? q.x : q.y;
  return __uint_as_float((i & 1) ? (pair & 0xffff0000u) : (pair << 16));
}

// Epilogue of the 3x3x3 convolutions (v2v_conv3, v2v_conv3_wide and v2v_conv3_deep inline it), one
// output value in the order of include/mvn_hip.h:
//   r = fma(acc, scale, shift) | + float(skip) | + fma(acc_s, scale_s, shift_s);  y = relu_keep_nan(r)
// for channel i (0..3) of the lane's four consecutive channels of one voxel.  sc, sh, scs, shs are
// anything indexable (registers, a vector, the global arrays), read at c0 + i; an operand that MODE
// does not use is never read.  The callers keep the loop over i and the 8-byte store of the four
// values: a helper that holds the loop is optimised before it is inlined and moves instructions in
// v2v_conv3_deep.
template <int MODE, typename S, typename SS>
__device__ __forceinline__ float bn_skip_relu(const f32x4_t& acc, const S& sc, const S& sh, const uint2& skip,
                                              const f32x4_t& accs, const SS& scs, const SS& shs, int i, int c0 = 0) {
  float r = __builtin_fmaf(acc[i], sc[c0 + i], sh[c0 + i]);
  if constexpr (MODE == MVN_SKIP_IDENTITY) r = r + bf16_of_pair(skip, i);
  if constexpr (MODE == MVN_SKIP_POINTWISE) r = r + __builtin_fmaf(accs[i], scs[c0 + i], shs[c0 + i]);
  return relu_keep_nan(r);
}

// Epilogue of the upsamples (v2v_upsample2, v2v_upsample2_deep), where the ReLU comes before the add:
//   y = relu_keep_nan(fma(acc, scale, shift)) + float(skip)
template <bool SKIP, typename S>
__device__ __forceinline__ float bn_relu_add(const f32x4_t& acc, const S& sc, const S& sh, const uint2& skip, int i,
                                             int c0 = 0) {
  float u = relu_keep_nan(__builtin_fmaf(acc[i], sc[c0 + i], sh[c0 + i]));
  if constexpr (SKIP) u = u + bf16_of_pair(skip, i);
  return u;
}

// Four consecutive channels rounded to bf16: the 8 bytes of one channels-last store.
__device__ __forceinline__ uint2 pack_bf16x4(const float (&y)[4]) {
  return make_uint2(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]));
}

// ---- host ------------------------------------------------------------------------------------
// The pointer checks that mvn_v2v_conv3, _wide and _deep make first: a null required pointer, an
// unknown skip_mode, or skip arguments that contradict the mode (given where it takes none, missing
// where it needs one) are MVN_ERR_ARG.
inline int check_conv3_pointers(const void* x, const void* wpk, const float* scale, const float* shift,
                                int skip_mode, const void* skip, const void* wskip, const float* scale_s,
                                const float* shift_s, const void* out) {
  if (!x || !wpk || !scale || !shift || !out) return MVN_ERR_ARG;
  if (skip_mode != MVN_SKIP_NONE && skip_mode != MVN_SKIP_IDENTITY && skip_mode != MVN_SKIP_POINTWISE)
    return MVN_ERR_ARG;
  const bool pw = wskip || scale_s || shift_s;
  if (skip_mode == MVN_SKIP_NONE && (skip || pw)) return MVN_ERR_ARG;
  if (skip_mode == MVN_SKIP_IDENTITY && (!skip || pw)) return MVN_ERR_ARG;
  if (skip_mode == MVN_SKIP_POINTWISE && (!skip || !wskip || !scale_s || !shift_s)) return MVN_ERR_ARG;
  return MVN_OK;
}

// f(std::integral_constant<int, MODE>) for a checked skip_mode: the kernels take it as a template
// argument.
template <typename F>
inline auto with_skip_mode(int skip_mode, F&& f) {
  if (skip_mode == MVN_SKIP_NONE) return f(std::integral_constant<int, MVN_SKIP_NONE>{});
  if (skip_mode == MVN_SKIP_IDENTITY) return f(std::integral_constant<int, MVN_SKIP_IDENTITY>{});
  return f(std::integral_constant<int, MVN_SKIP_POINTWISE>{});
}

}  // namespace mvn
