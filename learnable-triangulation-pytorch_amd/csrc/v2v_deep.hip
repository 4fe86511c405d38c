// The 128-channel levels of the V2V's encoder-decoder (16^3, 8^3, 4^3 and 2^3 at V = 64) on kernels
// for gfx950, eval mode, channels-last bf16 volumes on both sides:
//   mvn_v2v_conv3_deep     the 3x3x3 conv + folded BN + skip + ReLU of the Res3DBlocks with 128
//                          output channels: encoder_res2 (64 -> 128) and the twelve 128 -> 128 blocks
//                          from skip_res3 to decoder_res2
//   mvn_v2v_upsample2_deep decoder_upsample5..3 (ConvTranspose3d(128, 128, 2, 2) + BN + ReLU) and
//                          decoder_upsample2 (128 -> 64), each fused with the `+ skip` behind it
// (mvn/models/v2v.py:20-42, 53-65, 105-135).  The pools between the levels are
// v2v_interior.hip's mvn_v2v_maxpool2.  The arithmetic contracts are in include/mvn_hip.h.
//
// Any extent D in [1, 64].  Siblings of v2v_interior.hip's kernels with the same MFMA orientation
// (A = 16 output channels x 32 K-slots of one tap, B = 32 K-slots x 16 voxels, D = 16 channels x
// 16 voxels), but at these extents a tile of z-rows with a halo ring has nothing to walk along, so
// there is no LDS and no tile geometry: the voxels of all frames are flattened, B * D^3 of them, and
// cut into groups of 16, the MFMA's columns.  A group may span z-rows, x-slices and (D <= 2) frames:
// each lane derives (x, y, z) of its own voxel once, every tap gets a bounds predicate of its own,
// and a neighbour that passes it lies in the lane's own frame by construction.  Lanes past the
// last voxel neither read nor write.
//
// Conv.  A wave owns NG voxel groups x MTB channel tiles (NG * MTB accumulators) and walks the 27
// taps; per tap it loads its Cin/32 * MTB A fragments (1 KB each, contiguous, from the L2-resident
// packed weights) and its NG * Cin/32 B chunks (16 bytes per lane, straight from the volume, which
// is at most 1 MB per frame at 16^3), the next tap's into a second register set under the tap's
// MFMAs.  A fragment is used NG times, a chunk MTB times.  The host takes the largest of
// (NG, MTB) = (4, 4), (2, 4), (1, 2) that still gives one block per CU, so that 8 frames at 2^3 (4
// groups) are 16 waves and 8 frames at 16^3 stream the weights once per 64 voxels and half the
// channels.  No atomics, no split K: every output is one wave's sum in a fixed order.
//
// Upsample.  Per input voxel a 128 -> 8 * cout matrix product.  A wave owns one of the 8 output
// offsets: its 4 x cout/16 A fragments stay in registers (64 | 128 VGPRs) while it strides over the
// voxel groups; B = the 128 channels of 16 voxels read straight from global memory, one 8-byte skip
// load and one 8-byte store per channel tile.
#include <climits>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int CO = 128, NTAP = 27, MT = CO / 16;
constexpr int kWaves = 4, kThreads = kWaves * kWave;

template <int CIN, int MODE, int NG, int MTB>
__global__ __launch_bounds__(kThreads) void v2v_conv3_deep(
    const uint16_t* __restrict__ in, const uint4* __restrict__ wpk, const float* __restrict__ scale,
    const float* __restrict__ shift, const uint16_t* __restrict__ skip, const uint4* __restrict__ wskip,
    const float* __restrict__ scale_s, const float* __restrict__ shift_s, uint16_t* __restrict__ out, int D, int N,
    int nunits) {
  constexpr int KP = CIN / 32;                               // K-passes per tap
  constexpr int CH = CIN / 8;                                // 16-byte chunks per voxel record
  constexpr int CS = MT / MTB;                               // channel slices per voxel tile
  constexpr int kWChunks = NTAP * KP * MT * kWave;           // 16-byte chunks of the packed weights
  const int lane = threadIdx.x & (kWave - 1), c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  // units (voxel tile, channel slice), the slices of a tile adjacent; one per wave, XCD-contiguous.
  // No barrier in this kernel: a wave without a unit leaves.
  const int u = xcd_remap(blockIdx.x, gridDim.x) * kWaves + w;
  if (u >= nunits) return;
  const int vt = u / CS, m0 = (u % CS) * MTB;
  const int D2 = D * D, D3 = D2 * D;
  int v[NG];                                                 // the lane's voxel of group n, flattened over frames
  uint32_t pos[NG];                                          // x | y << 8 | z << 16 | (v < N) << 24
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    v[n] = (vt * NG + n) * 16 + c;
    const int r = v[n] % D3, x = r / D2, y = (r / D) % D, z = r % D;
    MVN_DASSERT(x < D && y < D && z < D && ((v[n] / D3) * D + x) * D2 + y * D + z == v[n]);
    pos[n] = uint32_t(x) | (uint32_t(y) << 8) | (uint32_t(z) << 16) | (v[n] < N ? 1u << 24 : 0u);
  }
  const uint4* in4 = reinterpret_cast<const uint4*>(in);

  // tap (dx, dy, dz): the wave's A fragments from [tap][kp][m][lane] and, per group, the lane's
  // chunks of voxel (x + dx - 1, y + dy - 1, z + dz - 1): zero outside the volume, which also keeps
  // the tap inside the lane's frame
  auto ldtap = [&](uint4 (&A)[KP][MTB], uint4 (&Bv)[NG][KP], int tap) {
    const int ox = tap / 9 - 1, oy = (tap / 3) % 3 - 1, oz = tap % 3 - 1;
#pragma unroll
    for (int kp = 0; kp < KP; ++kp)
#pragma unroll
      for (int ml = 0; ml < MTB; ++ml) {
        const int ai = ((tap * KP + kp) * MT + m0 + ml) * kWave + lane;
        MVN_DASSERT(tap >= 0 && tap < NTAP && ai >= 0 && ai < kWChunks);
        A[kp][ml] = wpk[ai];
      }
    const int dv = ox * D2 + oy * D + oz;
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      const int x = int(pos[n] & 255u) + ox, y = int((pos[n] >> 8) & 255u) + oy, z = int((pos[n] >> 16) & 255u) + oz;
      const bool ok = (pos[n] >> 24) && unsigned(x) < unsigned(D) && unsigned(y) < unsigned(D) &&
                      unsigned(z) < unsigned(D);
      const int nv = v[n] + dv;
      MVN_DASSERT(!ok || (nv >= 0 && nv < N && nv / D3 == v[n] / D3));
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) {
        Bv[n][kp] = make_uint4(0u, 0u, 0u, 0u);
        if (ok) Bv[n][kp] = in4[size_t(nv) * CH + 4 * kp + g];
      }
    }
  };
  f32x4_t acc[NG][MTB];
#pragma unroll
  for (int n = 0; n < NG; ++n)
#pragma unroll
    for (int ml = 0; ml < MTB; ++ml) acc[n][ml] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto fma_tap = [&](const uint4 (&A)[KP][MTB], const uint4 (&Bv)[NG][KP]) {
#pragma unroll
    for (int kp = 0; kp < KP; ++kp)
#pragma unroll
      for (int n = 0; n < NG; ++n)
#pragma unroll
        for (int ml = 0; ml < MTB; ++ml) acc[n][ml] = mfma(A[kp][ml], Bv[n][kp], acc[n][ml]);
  };

  uint4 A0[KP][MTB], A1[KP][MTB], B0[NG][KP], B1[NG][KP];
  ldtap(A0, B0, 0);
#pragma unroll 1
  for (int tap = 0; tap < NTAP; tap += 2) {
    if (tap + 1 < NTAP) ldtap(A1, B1, tap + 1);
    fma_tap(A0, B0);
    if (tap + 1 < NTAP) {
      if (tap + 2 < NTAP) ldtap(A0, B0, tap + 2);
      fma_tap(A1, B1);
    }
  }

  // ---- epilogue: folded BN, residual, ReLU (NaN kept, as F.relu), bf16, channels-last ----
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const bool ok = pos[n] >> 24;
    const size_t vo = size_t(v[n]);
    MVN_DASSERT(!ok || (v[n] >= 0 && v[n] < N));
    // POINTWISE: the lane's B chunks of the skip voxel.  The MFMAs run with every lane, in uniform
    // control flow (a lane past the end carries a zero column); only loads and stores are predicated.
    uint4 skb[2] = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
    if constexpr (MODE == MVN_SKIP_POINTWISE) {
      if (ok) {
        skb[0] = *reinterpret_cast<const uint4*>(skip + vo * 64 + 8 * g);
        skb[1] = *reinterpret_cast<const uint4*>(skip + vo * 64 + 32 + 8 * g);
      }
    }
#pragma unroll
    for (int ml = 0; ml < MTB; ++ml) {
      const int ch = 16 * (m0 + ml) + 4 * g;
      MVN_DASSERT(ch >= 0 && ch + 4 <= CO);
      f32x4_t accs = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MODE == MVN_SKIP_POINTWISE) {
        MVN_DASSERT((MT + m0 + ml) * kWave + lane < 2 * MT * kWave);
        accs = mfma(wskip[(m0 + ml) * kWave + lane], skb[0], accs);
        accs = mfma(wskip[(MT + m0 + ml) * kWave + lane], skb[1], accs);
      }
      if (!ok) continue;
      uint2 sk = make_uint2(0u, 0u);
      if constexpr (MODE == MVN_SKIP_IDENTITY) sk = *reinterpret_cast<const uint2*>(skip + vo * CO + ch);
      // bn_skip_relu (mfma.hpp) written out: through the helper, four of this kernel's instantiations
      // come out with two register quadruples exchanged
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float r = __builtin_fmaf(acc[n][ml][i], scale[ch + i], shift[ch + i]);
        if constexpr (MODE == MVN_SKIP_IDENTITY) r = r + bf16_of_pair(sk, i);
        if constexpr (MODE == MVN_SKIP_POINTWISE) r = r + __builtin_fmaf(accs[i], scale_s[ch + i], shift_s[ch + i]);
        y[i] = relu_keep_nan(r);
      }
      *reinterpret_cast<uint2*>(out + vo * CO + ch) = pack_bf16x4(y);
    }
  }
}

// ---------------------------------------------------------------------------- upsample
constexpr int UP_CI = 128, UP_KP = UP_CI / 32;
constexpr int kUpMaxStreams = 256;                           // x 8 offsets = 2048 waves, 512 blocks

template <int COUT, bool SKIP>
__global__ __launch_bounds__(kThreads) void v2v_upsample2_deep(const uint16_t* __restrict__ in,
                                                               const uint4* __restrict__ wpk,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const uint16_t* __restrict__ skip,
                                                               uint16_t* __restrict__ out, int D, int N, int ngroups,
                                                               int nstreams) {
  constexpr int H = COUT / 16;                               // channel tiles per offset
  constexpr int kUpChunks = UP_KP * 8 * H * kWave;
  const int lane = threadIdx.x & (kWave - 1), c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  // a wave: offset p = (dx * 2 + dy) * 2 + dz and one of nstreams strides over the voxel groups
  const int wg = blockIdx.x * kWaves + w, p = wg & 7, s = wg >> 3;
  if (s >= nstreams) return;
  uint4 A[UP_KP][H];
#pragma unroll
  for (int kp = 0; kp < UP_KP; ++kp)
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int ai = ((kp * 8 + p) * H + h) * kWave + lane;
      MVN_DASSERT(ai >= 0 && ai < kUpChunks);
      A[kp][h] = wpk[ai];
    }
  const int D2 = D * D, D3 = D2 * D;
  const size_t E = size_t(2 * D);
  const uint4* in4 = reinterpret_cast<const uint4*>(in);
  for (int grp = s; grp < ngroups; grp += nstreams) {
    const int v = grp * 16 + c;
    const bool ok = v < N;
    const int b = v / D3, r = v % D3, x = r / D2, y = (r / D) % D, z = r % D;
    MVN_DASSERT(!ok || (x < D && y < D && z < D && (b * D + x) * D2 + y * D + z == v));
    uint4 Bv[UP_KP];
#pragma unroll
    for (int kp = 0; kp < UP_KP; ++kp) {
      Bv[kp] = make_uint4(0u, 0u, 0u, 0u);
      if (ok) Bv[kp] = in4[size_t(v) * (UP_CI / 8) + 4 * kp + g];
    }
    const size_t ov = ((size_t(b) * E + size_t(2 * x + (p >> 2))) * E + size_t(2 * y + ((p >> 1) & 1))) * E +
                      size_t(2 * z + (p & 1));
    MVN_DASSERT(!ok || ov < size_t(N) * 8);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kp = 0; kp < UP_KP; ++kp) acc = mfma(A[kp][h], Bv[kp], acc);
      if (!ok) continue;
      const int ch = 16 * h + 4 * g;
      const size_t o = ov * COUT + ch;
      MVN_DASSERT(ch + 4 <= COUT && o + 4 <= size_t(N) * 8 * COUT);
      uint2 sk = make_uint2(0u, 0u);
      if constexpr (SKIP) sk = *reinterpret_cast<const uint2*>(skip + o);
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = bn_relu_add<SKIP>(acc, scale, shift, sk, i, ch);
      *reinterpret_cast<uint2*>(out + o) = pack_bf16x4(y);
    }
  }
}

// ---------------------------------------------------------------------------- host
constexpr int kDeepMaxD = 64;
constexpr int kCus = 256;

// B * D^3 voxels, or -1 where 8 times as many (the upsample's output voxels) overflow an int
long long deep_voxels(int B, int D) {
  const long long n = (long long)B * D * D * D;
  return n > INT_MAX / 8 ? -1 : n;
}

int blocks_of(int ngroups, int ng, int mtb) {
  const long long units = (long long)((ngroups + ng - 1) / ng) * (MT / mtb);
  return int((units + kWaves - 1) / kWaves);
}

template <int CIN, int MODE, int NG, int MTB>
void launch_deep_cfg(const void* x, const void* wpk, const float* scale, const float* shift, const void* skip,
                     const void* wskip, const float* scale_s, const float* shift_s, void* out, int D, int N,
                     hipStream_t st) {
  const int ngroups = (N + 15) / 16;
  const int nunits = ((ngroups + NG - 1) / NG) * (MT / MTB);
  v2v_conv3_deep<CIN, MODE, NG, MTB><<<blocks_of(ngroups, NG, MTB), kThreads, 0, st>>>(
      static_cast<const uint16_t*>(x), static_cast<const uint4*>(wpk), scale, shift,
      static_cast<const uint16_t*>(skip), static_cast<const uint4*>(wskip), scale_s, shift_s,
      static_cast<uint16_t*>(out), D, N, nunits);
}

// The largest wave tile that still gives every CU a block; the smallest one below that.
template <int CIN, int MODE>
int launch_deep(const void* x, const void* wpk, const float* scale, const float* shift, const void* skip,
                const void* wskip, const float* scale_s, const float* shift_s, void* out, int D, int N,
                hipStream_t st) {
  const int ngroups = (N + 15) / 16;
  if (blocks_of(ngroups, 4, 4) >= kCus)
    launch_deep_cfg<CIN, MODE, 4, 4>(x, wpk, scale, shift, skip, wskip, scale_s, shift_s, out, D, N, st);
  else if (blocks_of(ngroups, 2, 4) >= kCus)
    launch_deep_cfg<CIN, MODE, 2, 4>(x, wpk, scale, shift, skip, wskip, scale_s, shift_s, out, D, N, st);
  else
    launch_deep_cfg<CIN, MODE, 1, 2>(x, wpk, scale, shift, skip, wskip, scale_s, shift_s, out, D, N, st);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

template <int CIN>
int launch_deep_mode(int skip_mode, const void* x, const void* wpk, const float* scale, const float* shift,
                     const void* skip, const void* wskip, const float* scale_s, const float* shift_s, void* out,
                     int D, int N, hipStream_t st) {
  return with_skip_mode(skip_mode, [&](auto mode) {
    return launch_deep<CIN, decltype(mode)::value>(x, wpk, scale, shift, skip, wskip, scale_s, shift_s, out, D, N, st);
  });
}

template <int COUT>
int launch_up_deep(const void* x, const void* wpk, const float* scale, const float* shift, const void* skip,
                   void* out, int D, int N, hipStream_t st) {
  const int ngroups = (N + 15) / 16;
  const int nstreams = ngroups < kUpMaxStreams ? ngroups : kUpMaxStreams;
  const int nblk = (nstreams * 8 + kWaves - 1) / kWaves;
  const auto* in = static_cast<const uint16_t*>(x);
  const auto* wp = static_cast<const uint4*>(wpk);
  auto* o = static_cast<uint16_t*>(out);
  if (skip)
    v2v_upsample2_deep<COUT, true><<<nblk, kThreads, 0, st>>>(in, wp, scale, shift, static_cast<const uint16_t*>(skip),
                                                              o, D, N, ngroups, nstreams);
  else
    v2v_upsample2_deep<COUT, false><<<nblk, kThreads, 0, st>>>(in, wp, scale, shift, nullptr, o, D, N, ngroups,
                                                               nstreams);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_v2v_conv3_deep_packed_weight_bytes(int cin) {
  return cin == 64 || cin == 128 ? size_t(mvn::NTAP) * (cin / 32) * mvn::MT * mvn::kWave * 16 : 0;
}

extern "C" size_t mvn_v2v_conv3_deep_skip_packed_weight_bytes(int cin) {
  return cin == 64 ? size_t(2) * mvn::MT * mvn::kWave * 16 : 0;
}

extern "C" int mvn_v2v_conv3_deep(const void* x, int cin, const void* weight_packed, const float* scale,
                                  const float* shift, int skip_mode, const void* skip, int skip_cin,
                                  const void* skip_weight_packed, const float* skip_scale,
                                  const float* skip_shift, void* out, int B, int D, void* stream) {
  using namespace mvn;
  const int rc = check_conv3_pointers(x, weight_packed, scale, shift, skip_mode, skip, skip_weight_packed, skip_scale,
                                      skip_shift, out);
  if (rc != MVN_OK) return rc;
  if (B < 1 || D < 1 || D > kDeepMaxD || (cin != 64 && cin != 128)) return MVN_ERR_SHAPE;
  if (skip_mode == MVN_SKIP_IDENTITY && skip_cin != 128) return MVN_ERR_SHAPE;
  if (skip_mode == MVN_SKIP_POINTWISE && skip_cin != 64) return MVN_ERR_SHAPE;
  const long long n = deep_voxels(B, D);
  if (n < 0) return MVN_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return cin == 64 ? launch_deep_mode<64>(skip_mode, x, weight_packed, scale, shift, skip, skip_weight_packed,
                                          skip_scale, skip_shift, out, D, int(n), st)
                   : launch_deep_mode<128>(skip_mode, x, weight_packed, scale, shift, skip, skip_weight_packed,
                                           skip_scale, skip_shift, out, D, int(n), st);
}

extern "C" size_t mvn_v2v_upsample2_deep_packed_weight_bytes(int cout) {
  return cout == 64 || cout == 128 ? size_t(mvn::UP_KP) * 8 * (cout / 16) * mvn::kWave * 16 : 0;
}

extern "C" int mvn_v2v_upsample2_deep(const void* x, int cout, const void* weight_packed, const float* scale,
                                      const float* shift, const void* skip, void* out, int B, int D, void* stream) {
  using namespace mvn;
  if (!x || !weight_packed || !scale || !shift || !out) return MVN_ERR_ARG;
  if (B < 1 || D < 1 || D > kDeepMaxD || (cout != 64 && cout != 128)) return MVN_ERR_SHAPE;
  const long long n = deep_voxels(B, D);
  if (n < 0) return MVN_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return cout == 64 ? launch_up_deep<64>(x, weight_packed, scale, shift, skip, out, D, int(n), st)
                    : launch_up_deep<128>(x, weight_packed, scale, shift, skip, out, D, int(n), st);
}
