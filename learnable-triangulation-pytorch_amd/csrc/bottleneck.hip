// The convolutions of the 2-D backbone's ResNet trunk (mvn/models/pose_resnet.py:57-95, the Bottleneck
// of layer1 .. layer4), eval mode, on v_mfma_f32_16x16x32_bf16: the 1x1 convolution
// with a folded BatchNorm, the block's residual (identity, or the 1x1 strided downsample fused) and the
// ReLU behind it, and the 3x3 convolution with padding 1 and stride 1 or 2 with BatchNorm and ReLU.
// bf16 channels-last in and out.  The arithmetic contracts are in include/mvn_hip.h (mvn_conv1x1,
// mvn_conv3x3).
//
// Both are one implicit GEMM over the flat output pixels p = (n, oy, ox) of the whole batch: weights as
// A (D = 16 channels x 16 pixels, a lane holding 4 consecutive channels of one pixel: one 8-byte
// channels-last store), pixels as B.  A lane's B operand, the 8 channels 32 kp + 8 g .. + 7 of pixel c
// of a 16-pixel tile, is 16 contiguous bytes of the channels-last tensor, so it is loaded straight
// from global memory through the tensor's buffer resource, with no LDS between: for the 1x1 the pixel
// itself (or the pixel (s oy, s ox) of the skip tensor), for the 3x3 the pixel (s oy - 1 + ky,
// s ox - 1 + kx) of tap (ky, kx), at kOob (zero) where the tap lies outside the image or the pixel
// past the batch.  The weight fragments come from the packed tensor, 1 KB contiguous per fragment.
//
// Tile.  A wave takes 64 output channels x 64 pixels (4 x 4 accumulators, 64 registers) and per
// K-step of 32 loads 4 weight and 4 pixel fragments for 16 MFMAs, the next step's loads in flight
// under them.  A block is 4 waves on 4 consecutive 64-pixel tiles of one 64-channel group, so the
// weight fragments of a step are shared in L1; blocks of the same pixels and different channel groups
// are neighbours in the XCD's block order (xcd_remap), so the pixels are shared in L2.  The K-steps run
// tap-major for the 3x3 (9 C / 32 steps), in one fixed order for a launch.
#include <limits.h>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kMT = 4, kNT = 4;                      // 16-channel and 16-pixel tiles of a wave
constexpr int kGroupC = 16 * kMT;                    // 64 output channels of a block
constexpr int kWavePix = 16 * kNT, kBlockPix = kWaves * kWavePix;   // 64, 256
constexpr int kMinC = 64, kMaxC1 = 2048, kMaxC3 = 512;

// acc[ml][j] = the sum over the K-steps it = 0 .. iters - 1 (iters even) of A(it, m0 + ml) x B(it, j):
// A from wpk as [it][m 0..mtiles-1][lane], B the 16 bytes at byte offset off(it, j) behind rs.
template <typename OffF>
__device__ __forceinline__ void mfma_loop(const __amdgpu_buffer_rsrc_t rs, const uint4* __restrict__ wpk, int mtiles,
                                          int m0, int iters, int lane, OffF off, f32x4_t (&acc)[kMT][kNT]) {
  auto load = [&](int it, uint4 (&A)[kMT], uint4 (&B)[kNT]) {
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) {
      const int ai = ((it * mtiles) + m0 + ml) * kWave + lane;
      MVN_DASSERT(it >= 0 && it < iters && m0 + ml < mtiles && ai >= 0);
      A[ml] = wpk[ai];
    }
#pragma unroll
    for (int j = 0; j < kNT; ++j)
      B[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off(it, j), 0, 0));
  };
  auto mma = [&](const uint4 (&A)[kMT], const uint4 (&B)[kNT]) {
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml)
#pragma unroll
      for (int j = 0; j < kNT; ++j) acc[ml][j] = mfma(A[ml], B[j], acc[ml][j]);
  };
#pragma unroll
  for (int ml = 0; ml < kMT; ++ml)
#pragma unroll
    for (int j = 0; j < kNT; ++j) acc[ml][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  uint4 A0[kMT], B0[kNT], A1[kMT], B1[kNT];
  load(0, A0, B0);
#pragma unroll 1
  for (int it = 0; it < iters; it += 2) {
    load(it + 1, A1, B1);
    __builtin_amdgcn_sched_barrier(0);               // the next step's loads are requested before this step's MFMAs
    mma(A0, B0);
    __builtin_amdgcn_sched_barrier(0);
    load(it + 2 < iters ? it + 2 : it, A0, B0);      // past the end: a step again, in bounds, unused
    __builtin_amdgcn_sched_barrier(0);
    mma(A1, B1);
  }
}

// The block's channel group and the wave's first pixel from the block index.
__device__ __forceinline__ void tile_of_block(int groups, int& cg, int& p0) {
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  cg = L % groups;
  p0 = (L / groups) * kBlockPix + w * kWavePix;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void conv1x1(const uint16_t* __restrict__ x, const uint4* __restrict__ wpk,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const uint16_t* __restrict__ skip, const uint4* __restrict__ wsk,
                                                    const float* __restrict__ scale_s,
                                                    const float* __restrict__ shift_s, uint16_t* __restrict__ out,
                                                    int P, int cin, int cout, int H, int W, int cs, int Hs, int Ws,
                                                    int sstride) {
  const int lane = threadIdx.x & (kWave - 1), c = lane & 15, g = lane >> 4;
  int cg, p0;
  tile_of_block(cout / kGroupC, cg, p0);
  if (p0 >= P) return;                               // no barrier in this kernel: a wave may leave

  f32x4_t acc[kMT][kNT], accs[kMT][kNT];
  if constexpr (MODE == MVN_SKIP_POINTWISE) {
    // the downsample: pixel (n, oy, ox) reads pixel (n, s oy, s ox) of the (M, Hs, Ws, cs) skip tensor
    const __amdgpu_buffer_rsrc_t rss = make_rsrc(skip, uint32_t(P / (H * W)) * uint32_t(Hs * Ws) * uint32_t(cs) * 2u);
    uint32_t soff[kNT];
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const int p = p0 + 16 * j + c;
      const int n = p / (H * W), rem = p - n * (H * W);
      const int oy = rem / W, ox = rem - oy * W;
      const int sp = (n * Hs + sstride * oy) * Ws + sstride * ox;
      MVN_DASSERT(p >= P || (sstride * oy < Hs && sstride * ox < Ws));
      soff[j] = p < P ? uint32_t(sp) * uint32_t(cs) * 2u + 16u * g : kOob;
    }
    mfma_loop(rss, wsk, cout / 16, cg * kMT, cs / 32, lane, [&](int it, int j) { return soff[j] + uint32_t(it) * 64u; },
              accs);
  }
  {
    const __amdgpu_buffer_rsrc_t rsx = make_rsrc(x, uint32_t(P) * uint32_t(cin) * 2u);
    uint32_t xoff[kNT];
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const int p = p0 + 16 * j + c;
      xoff[j] = p < P ? uint32_t(p) * uint32_t(cin) * 2u + 16u * g : kOob;
    }
    mfma_loop(rsx, wpk, cout / 16, cg * kMT, cin / 32, lane, [&](int it, int j) { return xoff[j] + uint32_t(it) * 64u; },
              acc);
  }

  // ---- epilogue: folded BN, the skip term, ReLU (NaN kept), one rounding, predicated 8-byte stores ----
  // lane: channels co + i of pixel p0 + 16 j + c
#pragma unroll
  for (int ml = 0; ml < kMT; ++ml) {
    const int co = cg * kGroupC + 16 * ml + 4 * g;
    const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(scale + co);
    const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(shift + co);
    f32x4_t scs = sc, shs = sh;
    if constexpr (MODE == MVN_SKIP_POINTWISE) {
      scs = *reinterpret_cast<const f32x4_t*>(scale_s + co);
      shs = *reinterpret_cast<const f32x4_t*>(shift_s + co);
    }
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const int p = p0 + 16 * j + c;
      if (p >= P) continue;
      const size_t o = size_t(p) * cout + co;
      uint2 sk = make_uint2(0u, 0u);
      if constexpr (MODE == MVN_SKIP_IDENTITY) sk = *reinterpret_cast<const uint2*>(skip + o);
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        y[i] = bn_skip_relu<MODE>(acc[ml][j], sc, sh, sk, MODE == MVN_SKIP_POINTWISE ? accs[ml][j] : acc[ml][j], scs, shs, i);
      *reinterpret_cast<uint2*>(out + o) = pack_bf16x4(y);
    }
  }
}

__global__ __launch_bounds__(kThreads) void conv3x3(const uint16_t* __restrict__ x, const uint4* __restrict__ wpk,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    uint16_t* __restrict__ out, int P, int C, int H, int W, int Ho,
                                                    int Wo, int stride) {
  const int lane = threadIdx.x & (kWave - 1), c = lane & 15, g = lane >> 4;
  int cg, p0;
  tile_of_block(C / kGroupC, cg, p0);
  if (p0 >= P) return;

  // the lane's four output pixels: the input pixel of tap (0, 0) and its flat index in x (may be
  // negative: used only where the tap is inside the image)
  const __amdgpu_buffer_rsrc_t rsx = make_rsrc(x, uint32_t(P / (Ho * Wo)) * uint32_t(H * W) * uint32_t(C) * 2u);
  int iy0[kNT], ix0[kNT], pix0[kNT];
  bool live[kNT];
#pragma unroll
  for (int j = 0; j < kNT; ++j) {
    const int p = p0 + 16 * j + c;
    live[j] = p < P;
    const int q = live[j] ? p : 0;
    const int n = q / (Ho * Wo), rem = q - n * (Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    iy0[j] = stride * oy - 1;
    ix0[j] = stride * ox - 1;
    pix0[j] = (n * H + iy0[j]) * W + ix0[j];
  }
  const int KP = C / 32;
  const float inv_kp = 1.0f / float(KP);
  auto off = [&](int it, int j) -> uint32_t {
    const int tap = int((float(it) + 0.5f) * inv_kp);    // it / KP: it < 144, KP <= 16
    const int kp = it - tap * KP;
    const int ky = tap / 3, kx = tap - 3 * ky;
    MVN_DASSERT(tap >= 0 && tap < 9 && kp >= 0 && kp < KP);
    const bool ok = live[j] & (unsigned(iy0[j] + ky) < unsigned(H)) & (unsigned(ix0[j] + kx) < unsigned(W));
    return ok ? uint32_t(pix0[j] + ky * W + kx) * (uint32_t(C) * 2u) + 16u * g + uint32_t(kp) * 64u : kOob;
  };
  f32x4_t acc[kMT][kNT];
  mfma_loop(rsx, wpk, C / 16, cg * kMT, 9 * KP, lane, off, acc);

#pragma unroll
  for (int ml = 0; ml < kMT; ++ml) {
    const int co = cg * kGroupC + 16 * ml + 4 * g;
    const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(scale + co);
    const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(shift + co);
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const int p = p0 + 16 * j + c;
      if (p >= P) continue;
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        y[i] = bn_skip_relu<MVN_SKIP_NONE>(acc[ml][j], sc, sh, make_uint2(0u, 0u), acc[ml][j], sc, sh, i);
      *reinterpret_cast<uint2*>(out + size_t(p) * C + co) = pack_bf16x4(y);
    }
  }
}

inline bool channels_ok(int c, int max_c) { return c >= kMinC && c <= max_c && c % 64 == 0; }

// n_images * H * W pixels of `channels` bf16 below 2^31 bytes; the pixel count in *pixels.
inline bool tensor_fits(int64_t n_images, int H, int W, int channels, long long* pixels) {
  if (n_images > INT_MAX) return false;
  long long p = (long long)n_images * H;
  if (p > INT_MAX) return false;
  p *= W;
  if (p > INT_MAX || p * channels * 2 > (long long)INT_MAX) return false;
  *pixels = p;
  return true;
}

inline bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_conv1x1_packed_weight_bytes(int cin, int cout) {
  using namespace mvn;
  return channels_ok(cin, kMaxC1) && channels_ok(cout, kMaxC1) ? size_t(cin / 32) * (cout / 16) * kWave * 16 : 0;
}

extern "C" int mvn_conv1x1(const void* x, const void* weight_packed, const float* scale, const float* shift,
                           int skip_mode, const void* skip, const void* skip_weight_packed, const float* skip_scale,
                           const float* skip_shift, int skip_cin, int skip_H, int skip_W, int skip_stride, void* out,
                           int64_t n_images, int H, int W, int cin, int cout, void* stream) {
  using namespace mvn;
  if (check_conv3_pointers(x, weight_packed, scale, shift, skip_mode, skip, skip_weight_packed, skip_scale, skip_shift,
                           out) != MVN_OK)
    return MVN_ERR_ARG;
  if (!channels_ok(cin, kMaxC1) || !channels_ok(cout, kMaxC1)) return MVN_ERR_ARG;
  if (n_images < 0 || H < 1 || W < 1) return MVN_ERR_ARG;
  if (!aligned16({x, weight_packed, scale, shift, skip, skip_weight_packed, skip_scale, skip_shift, out}))
    return MVN_ERR_ARG;
  long long P, Pout, Ps = 0;
  if (!tensor_fits(n_images, H, W, cin, &P) || !tensor_fits(n_images, H, W, cout, &Pout)) return MVN_ERR_ARG;
  if (skip_mode == MVN_SKIP_POINTWISE) {
    if (!channels_ok(skip_cin, kMaxC1) || (skip_stride != 1 && skip_stride != 2) || skip_H < 1 || skip_W < 1)
      return MVN_ERR_ARG;
    if (H != (skip_H - 1) / skip_stride + 1 || W != (skip_W - 1) / skip_stride + 1) return MVN_ERR_ARG;
    if (!tensor_fits(n_images, skip_H, skip_W, skip_cin, &Ps)) return MVN_ERR_ARG;
  }
  if (n_images == 0) return MVN_OK;
  const long long blocks = ((P + kBlockPix - 1) / kBlockPix) * (cout / kGroupC);   // below 2^31 / 128 * 32
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_skip_mode(skip_mode, [&](auto mode) {
    conv1x1<decltype(mode)::value><<<int(blocks), kThreads, 0, st>>>(
        static_cast<const uint16_t*>(x), static_cast<const uint4*>(weight_packed), scale, shift,
        static_cast<const uint16_t*>(skip), static_cast<const uint4*>(skip_weight_packed), skip_scale, skip_shift,
        static_cast<uint16_t*>(out), int(P), cin, cout, H, W, skip_cin, skip_H, skip_W, skip_stride);
  });
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" size_t mvn_conv3x3_packed_weight_bytes(int channels) {
  using namespace mvn;
  return channels_ok(channels, kMaxC3) ? size_t(9) * (channels / 32) * (channels / 16) * kWave * 16 : 0;
}

extern "C" int mvn_conv3x3(const void* x, const void* weight_packed, const float* scale, const float* shift, void* out,
                           int64_t n_images, int H, int W, int channels, int stride, void* stream) {
  using namespace mvn;
  if (!x || !weight_packed || !scale || !shift || !out) return MVN_ERR_ARG;
  if (!channels_ok(channels, kMaxC3) || (stride != 1 && stride != 2)) return MVN_ERR_ARG;
  if (n_images < 0 || H < 1 || W < 1) return MVN_ERR_ARG;
  if (!aligned16({x, weight_packed, scale, shift, out})) return MVN_ERR_ARG;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  long long Pin, P;
  if (!tensor_fits(n_images, H, W, channels, &Pin) || !tensor_fits(n_images, Ho, Wo, channels, &P)) return MVN_ERR_ARG;
  if (n_images == 0) return MVN_OK;
  const long long blocks = ((P + kBlockPix - 1) / kBlockPix) * (channels / kGroupC);
  conv3x3<<<int(blocks), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint16_t*>(x), static_cast<const uint4*>(weight_packed), scale, shift,
      static_cast<uint16_t*>(out), int(P), channels, H, W, Ho, Wo, stride);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}
