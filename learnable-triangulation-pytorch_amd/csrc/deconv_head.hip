// The deconv head of the 2-D backbone (mvn/models/pose_resnet.py:266-291): one
// ConvTranspose2d(Cin, 256, 4, stride 2, padding 1, bias=False) + BatchNorm2d + ReLU per launch,
// eval mode, on v_mfma_f32_16x16x32_bf16, and the last layer with the volumetric
// model's Conv2d(256, 32, 1) behind it in the same launch.  The arithmetic
// contracts are in include/mvn_hip.h (mvn_deconv4s2, mvn_deconv4s2_project).
//
// Decomposition.  Output (oy, ox) = (2 r + py, 2 c + px) of input pixel (r, c) and parity (py, px)
// takes the 2 x 2 taps whose ky has the parity of py + 1 and whose kx has that of px + 1:
//   ky = 1 -> input row r      ky = 3 -> row r - 1      (py = 0)
//   ky = 0 -> input row r + 1  ky = 2 -> row r          (py = 1)
// and the same along x, so each parity is one implicit GEMM with K = 4 Cin over the input pixels
// and their one-pixel halo ring, and every tap belongs to exactly one parity.
//
// Tile.  A block takes 4 x 16 input pixels of one image and 128 of the 256 output channels, all
// four parities: 8 x 32 output pixels.  Its 6 x 18-pixel halo of one 32-channel K-chunk (432 chunks
// of 16 bytes, 6,912 B) is staged once per chunk into one of two LDS buffers, the next chunk's
// loads in flight under the MFMAs; a pixel outside the image is loaded at kOob through the image's
// buffer resource and is zero.  Wave w of the 4 takes output channels 32 w .. 32 w + 31 of the
// block's half (2 channel tiles) for all 4 rows: 4 parities x 2 tiles x 4 rows = 32 accumulators
// (128 registers).  Per K-chunk it reads the 6 x 3 pixel fragments (halo row, x shift) from LDS
// once (one fragment = the 16 pixels of a row at one shift, 1 KB contiguous: conflict-free) and
// the 16 x 2 weight fragments straight from the packed tensor in global memory (each is used by
// one wave of the block only, 1 KB contiguous), one ky row of 8 fragments ahead of its 32 MFMAs.
//
// Layouts.  The two MFMA operands have the same register layout, so the output layout is the
// operand order: weights as A gives D = 16 channels x 16 pixels, a lane holding 4 consecutive
// channels of one pixel (one 8-byte channels-last store); pixels as A gives D = 16 pixels x 16
// channels, a lane holding 4 x-consecutive input pixels of one channel, which with both x-parities
// are 8 consecutive outputs of one NCHW row (one 16-byte bf16 store or two 16-byte f32 stores where
// W % 4 == 0, single elements otherwise).  Each output element is the same 4 Cin / 32 MFMA sums in
// the same order either way.
#include <limits.h>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int kCout = 256;
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int TH = 4, TW = 16;                       // input pixels of a block's tile
constexpr int HH = TH + 2, HW_ = TW + 2;             // with the halo ring: 6 x 18
constexpr int kHaloChunks = HH * HW_ * 4;            // 16-byte chunks of one 32-channel K-chunk: 432
constexpr int kStage = (kHaloChunks + kThreads - 1) / kThreads;   // chunks a thread stages: 2
constexpr int kMT = 2;                               // 16-channel tiles of a wave
constexpr int kBlockCout = kWaves * kMT * 16;        // 128
constexpr int kMinCin = 32, kMaxCin = 2048;

// parity and input offset of tap index k (ky or kx)
__device__ __forceinline__ constexpr int tap_parity(int k) { return (k + 1) & 1; }
__device__ __forceinline__ constexpr int tap_shift(int k) { return (tap_parity(k) + 1 - k) / 2; }   // -1, 0, +1

// The main loop that mvn_deconv4s2 and mvn_deconv4s2_project share: the 4 x 16-pixel tile at (y0, x0) of
// the image behind rs, all four parities, the wave's channel tiles m0, m0 + 1 of 16, summed over the
// cin / 32 K-chunks into acc (zeroed here).  NCHW is the operand order: pixels as A (D = 16 pixels x
// 16 channels) or weights as A (D = 16 channels x 16 pixels); an element's MFMA sums and their order
// are the same either way.  The caller's threads must all be past their last read of halo.
template <bool NCHW>
__device__ __forceinline__ void deconv_tile(uint4 (&halo)[2][kHaloChunks], const __amdgpu_buffer_rsrc_t rs,
                                            const uint4* __restrict__ wpk, int H, int W, int cin, int y0, int x0,
                                            int m0, f32x4_t (&acc)[4][kMT][TH]) {
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int c = lane & 15, g = lane >> 4;
  const int KP = cin / 32;
  uint32_t soff[kStage];                             // byte offset of the thread's chunks at K-chunk 0
#pragma unroll
  for (int u = 0; u < kStage; ++u) {
    const int q = t + u * kThreads, px = q >> 2, ch = q & 3;
    const int hy = px / HW_, hx = px - hy * HW_;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    const bool ok = (q < kHaloChunks) & (unsigned(gy) < unsigned(H)) & (unsigned(gx) < unsigned(W));
    soff[u] = ok ? (uint32_t(gy * W + gx) * uint32_t(cin) + 8u * ch) * 2u : kOob;
  }
  auto stage_load = [&](int kp, uint4 (&sv)[kStage]) {
#pragma unroll
    for (int u = 0; u < kStage; ++u)
      sv[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, soff[u] + uint32_t(kp) * 64u, 0, 0));
  };
  auto stage_store = [&](int buf, const uint4 (&sv)[kStage]) {
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int q = t + u * kThreads;
      MVN_DASSERT(buf >= 0 && buf < 2);
      if (q < kHaloChunks) halo[buf][q] = sv[u];
    }
  };

  // the 4 kx x kMT fragments of tap row ky of K-chunk kp, from [tap][kp][m][lane]
  auto load_a = [&](int kp, int ky, uint4 (&A)[4][kMT]) {
#pragma unroll
    for (int kx = 0; kx < 4; ++kx)
#pragma unroll
      for (int ml = 0; ml < kMT; ++ml) {
        const int ai = (((ky * 4 + kx) * KP + kp) * (kCout / 16) + m0 + ml) * kWave + lane;
        MVN_DASSERT(ai >= 0 && ai < 16 * KP * (kCout / 16) * kWave);
        A[kx][ml] = wpk[ai];
      }
  };

#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml)
#pragma unroll
      for (int r = 0; r < TH; ++r) acc[p][ml][r] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  uint4 sv[kStage];
  uint4 A[2][4][kMT];
  stage_load(0, sv);
  load_a(0, 0, A[0]);
  stage_store(0, sv);

#pragma unroll 1
  for (int kp = 0; kp < KP; ++kp) {
    __syncthreads();                                 // K-chunk kp is in halo[kp & 1]; kp - 1's readers are done
    const int kpn = kp + 1 < KP ? kp + 1 : kp;
    if (kp + 1 < KP) stage_load(kp + 1, sv);
    // the lane's pixel fragments: halo row hy, pixel x0 - 1 + c + dxi, channels 8 g .. 8 g + 7
    uint4 Bf[HH][3];
    const uint4* hb = halo[kp & 1];
#pragma unroll
    for (int hy = 0; hy < HH; ++hy)
#pragma unroll
      for (int dxi = 0; dxi < 3; ++dxi) {
        const int li = (hy * HW_ + c + dxi) * 4 + g;
        MVN_DASSERT(li >= 0 && li < kHaloChunks);
        Bf[hy][dxi] = hb[li];
      }
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      __builtin_amdgcn_sched_barrier(0);             // the next row's fragments are requested before this row's MFMAs
      if (ky + 1 < 4)
        load_a(kp, ky + 1, A[(ky + 1) & 1]);
      else
        load_a(kpn, 0, A[0]);
      __builtin_amdgcn_sched_barrier(0);
      const int py = tap_parity(ky), dy = tap_shift(ky);
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int px = tap_parity(kx), dx = tap_shift(kx);
#pragma unroll
        for (int ml = 0; ml < kMT; ++ml)
#pragma unroll
          for (int r = 0; r < TH; ++r) {
            f32x4_t& a = acc[py * 2 + px][ml][r];
            if constexpr (NCHW)
              a = mfma(Bf[r + 1 + dy][1 + dx], A[ky & 1][kx][ml], a);      // D: 16 pixels x 16 channels
            else
              a = mfma(A[ky & 1][kx][ml], Bf[r + 1 + dy][1 + dx], a);      // D: 16 channels x 16 pixels
          }
      }
    }
    if (kp + 1 < KP) stage_store((kp + 1) & 1, sv);
  }
}

// The NCHW store of both kernels: y = the outputs 2 ix0 .. 2 ix0 + 7 of one row of one channel, at o.
// vec (W % 4 == 0): the 8 are inside the row or all outside it, and o is 16-byte aligned.
template <typename TO>
__device__ __forceinline__ void store_row8(TO* o, const float (&y)[8], int vec, int ix0, int W) {
  if (vec) {
    if (ix0 >= W) return;
    MVN_DASSERT(ix0 + 3 < W && reinterpret_cast<uintptr_t>(o) % 16 == 0);
    if constexpr (sizeof(TO) == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(y[0], y[1], y[2], y[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(y[4], y[5], y[6], y[7]);
    } else {
      *reinterpret_cast<uint4*>(o) = make_uint4(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]),
                                                pack_bf16x2(y[4], y[5]), pack_bf16x2(y[6], y[7]));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (ix0 + (k >> 1) < W) store_elem<TO>(o + k, y[k]);
  }
}

template <bool NCHW, typename TO>
__global__ __launch_bounds__(kThreads) void deconv4s2(const uint16_t* __restrict__ x, const uint4* __restrict__ wpk,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ shift, TO* __restrict__ out, int H,
                                                      int W, int cin, int nTy, int nTx, int vec) {
  __shared__ uint4 halo[2][kHaloChunks];             // [buffer][hy][hx][chunk of 8 channels]
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(t / kWave);
  const int c = lane & 15, g = lane >> 4;
  int L = blockIdx.x;
  const int half = L & 1; L >>= 1;
  const int tx = L % nTx; L /= nTx;
  const int ty = L % nTy;
  const int n = L / nTy;
  const int y0 = ty * TH, x0 = tx * TW;
  // one image per resource: a halo pixel outside the image reads zero, never the neighbouring image
  const __amdgpu_buffer_rsrc_t rs =
      make_rsrc(x + size_t(n) * H * W * cin, uint32_t(H) * uint32_t(W) * uint32_t(cin) * 2u);

  f32x4_t acc[4][kMT][TH];                           // [parity py * 2 + px][channel tile][row]
  // the wave's channel tiles of the packed weight: m0, m0 + 1 of 16
  deconv_tile<NCHW>(halo, rs, wpk, H, W, cin, y0, x0, half * (kBlockCout / 16) + w * kMT, acc);

  // ---- epilogue: folded BN, ReLU (NaN kept, as F.relu), one rounding, predicated stores ----
  const int H2 = 2 * H, W2 = 2 * W;
  const int co0 = half * kBlockCout + w * kMT * 16;
  if constexpr (NCHW) {
    // lane: channel co0 + 16 ml + c, input pixels x0 + 4 g + i of row y0 + r
    const int ix0 = x0 + 4 * g;
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) {
      const int co = co0 + 16 * ml + c;
      const float sc = scale[co], sh = shift[co];
      TO* oc = out + (size_t(n) * kCout + co) * H2 * W2;
#pragma unroll
      for (int r = 0; r < TH; ++r) {
        if (y0 + r >= H) continue;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          float y[8];                                // outputs 2 ix0 .. 2 ix0 + 7 of row 2 (y0 + r) + py
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int px = 0; px < 2; ++px)
              y[2 * i + px] = relu_keep_nan(__builtin_fmaf(acc[py * 2 + px][ml][r][i], sc, sh));
          store_row8<TO>(oc + size_t(2 * (y0 + r) + py) * W2 + 2 * ix0, y, vec, ix0, W);
        }
      }
    }
  } else {
    // lane: channels co0 + 16 ml + 4 g + i of input pixel x0 + c of row y0 + r
    const int ix = x0 + c;
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) {
      const int co = co0 + 16 * ml + 4 * g;
      const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(scale + co);
      const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(shift + co);
#pragma unroll
      for (int r = 0; r < TH; ++r) {
        if (y0 + r >= H || ix >= W) continue;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int oy = 2 * (y0 + r) + (p >> 1), ox = 2 * ix + (p & 1);
          float y[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = relu_keep_nan(__builtin_fmaf(acc[p][ml][r][i], sc[i], sh[i]));
          MVN_DASSERT(oy < H2 && ox < W2);
          *reinterpret_cast<uint2*>(out + ((size_t(n) * H2 + oy) * W2 + ox) * kCout + co) = pack_bf16x4(y);
        }
      }
    }
  }
}

// ---- the last layer with the 256 -> 32 projection behind it (mvn_deconv4s2_project) ----
// A block takes the same 4 x 16-pixel tile and both channel halves, one after the other through
// deconv_tile in the weights-as-A order: a lane then holds channels {4 g + i, 16 + 4 g + i} of the wave's
// 32 for pixel c of each (parity, row), which after BN, ReLU and the rounding to bf16 are the 8 K-slots
// of an MFMA operand (the projection weight is packed with the same permutation).  The four waves
// exchange these fragments through LDS, [row][parity][wave][lane], 64 KB: wave w then owns tile row w
// and projects it over the half's 128 channels, activations as A (D = 16 pixels x 16 output
// channels, the layout of the NCHW store).  Its 8 accumulators (4 parities x 2 tiles of 16 output
// channels) start at the bias and take, per half and per 32-channel group in ascending order, the hi
// product and then the lo product: one fixed chain per output, whatever the grid.
constexpr int kProj = 32, kPT = kProj / 16;          // output channels of the projection, tiles of 16
constexpr int kGroups = kCout / 32;                  // 32-channel K-groups of the projection: 8

template <typename TO>
__global__ __launch_bounds__(kThreads) void deconv4s2_project(const uint16_t* __restrict__ x,
                                                              const uint4* __restrict__ wpk,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift,
                                                              const uint4* __restrict__ ppk,
                                                              const float* __restrict__ bias, TO* __restrict__ out,
                                                              int H, int W, int cin, int nTy, int nTx, int vec) {
  __shared__ uint4 halo[2][kHaloChunks];             // [buffer][hy][hx][chunk of 8 channels]
  __shared__ uint4 xch[TH][4][kWaves][kWave];        // [row][parity][wave = 32-channel group of the half][lane]
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(t / kWave);
  const int c = lane & 15, g = lane >> 4;
  int L = blockIdx.x;
  const int tx = L % nTx; L /= nTx;
  const int ty = L % nTy;
  const int n = L / nTy;
  const int y0 = ty * TH, x0 = tx * TW;
  const __amdgpu_buffer_rsrc_t rs =
      make_rsrc(x + size_t(n) * H * W * cin, uint32_t(H) * uint32_t(W) * uint32_t(cin) * 2u);

  f32x4_t S[4][kPT];                                 // [parity][output tile]: pixels x0 + 4 g + i of row y0 + w
#pragma unroll
  for (int nt = 0; nt < kPT; ++nt) {
    const float b = bias[16 * nt + c];
#pragma unroll
    for (int p = 0; p < 4; ++p) S[p][nt] = f32x4_t{b, b, b, b};
  }

#pragma unroll 1
  for (int half = 0; half < kCout / kBlockCout; ++half) {
    f32x4_t acc[4][kMT][TH];                         // [parity py * 2 + px][channel tile][row]
    deconv_tile<false>(halo, rs, wpk, H, W, cin, y0, x0, half * (kBlockCout / 16) + w * kMT, acc);

    // the projection's fragments of this half, [part hi | lo][group][tile][lane], in flight under the exchange
    uint4 P[kWaves][2][kPT];
#pragma unroll
    for (int k = 0; k < kWaves; ++k)
#pragma unroll
      for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int nt = 0; nt < kPT; ++nt) {
          const int pi = ((part * kGroups + half * kWaves + k) * kPT + nt) * kWave + lane;
          MVN_DASSERT(pi >= 0 && pi < 2 * kGroups * kPT * kWave);
          P[k][part][nt] = ppk[pi];
        }

    // the activation as mvn_deconv4s2 rounds it: channels co + i and co + 16 + i of pixel c
    const int co = half * kBlockCout + w * kMT * 16 + 4 * g;
    f32x4_t sc[kMT], sh[kMT];
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) {
      sc[ml] = *reinterpret_cast<const f32x4_t*>(scale + co + 16 * ml);
      sh[ml] = *reinterpret_cast<const f32x4_t*>(shift + co + 16 * ml);
    }
#pragma unroll
    for (int r = 0; r < TH; ++r)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        uint2 q[kMT];
#pragma unroll
        for (int ml = 0; ml < kMT; ++ml) {
          float y[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = relu_keep_nan(__builtin_fmaf(acc[p][ml][r][i], sc[ml][i], sh[ml][i]));
          q[ml] = pack_bf16x4(y);
        }
        MVN_DASSERT(w >= 0 && w < kWaves);
        xch[r][p][w][lane] = make_uint4(q[0].x, q[0].y, q[1].x, q[1].y);
      }
    __syncthreads();                                 // also: every wave is past its last read of halo

#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      uint4 a[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) a[p] = xch[w][p][k][lane];
#pragma unroll
      for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int nt = 0; nt < kPT; ++nt) S[p][nt] = mfma(a[p], P[k][part][nt], S[p][nt]);
    }
    // the next half's K-loop has a barrier between these reads of xch and its writes
  }

  // lane: output channel 16 nt + c, input pixels x0 + 4 g + i of row y0 + w
  if (y0 + w >= H) return;
  const int H2 = 2 * H, W2 = 2 * W, ix0 = x0 + 4 * g;
#pragma unroll
  for (int nt = 0; nt < kPT; ++nt) {
    TO* oc = out + (size_t(n) * kProj + 16 * nt + c) * H2 * W2;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      float y[8];                                    // outputs 2 ix0 .. 2 ix0 + 7 of row 2 (y0 + w) + py
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int px = 0; px < 2; ++px) y[2 * i + px] = S[py * 2 + px][nt][i];
      store_row8<TO>(oc + size_t(2 * (y0 + w) + py) * W2 + 2 * ix0, y, vec, ix0, W);
    }
  }
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_deconv4s2_packed_weight_bytes(int cin) {
  using namespace mvn;
  return cin >= kMinCin && cin <= kMaxCin && cin % 32 == 0 ? size_t(16) * (cin / 32) * (kCout / 16) * kWave * 16 : 0;
}

extern "C" int mvn_deconv4s2(const void* x, const void* weight_packed, const float* scale, const float* shift,
                             void* out, int out_layout, int out_dtype, int64_t n_images, int cin, int H, int W,
                             void* stream) {
  using namespace mvn;
  if (!x || !weight_packed || !scale || !shift || !out) return MVN_ERR_ARG;
  if (out_layout != MVN_LAYOUT_NCHW && out_layout != MVN_LAYOUT_NHWC) return MVN_ERR_ARG;
  if (out_dtype != MVN_DTYPE_F32 && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (out_layout == MVN_LAYOUT_NHWC && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (cin < kMinCin || cin > kMaxCin || cin % 32 != 0) return MVN_ERR_ARG;
  if (n_images < 0 || H < 1 || W < 1) return MVN_ERR_ARG;
  const auto xa = reinterpret_cast<uintptr_t>(x), wa = reinterpret_cast<uintptr_t>(weight_packed);
  const auto oa = reinterpret_cast<uintptr_t>(out);
  if (xa % 16 != 0 || wa % 16 != 0 || oa % 16 != 0) return MVN_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(scale) % 16 != 0 || reinterpret_cast<uintptr_t>(shift) % 16 != 0) return MVN_ERR_ARG;
  // one image fits a buffer resource on both sides: the input's cin * H * W bf16 and the output's
  // 256 * 2H * 2W elements of up to 4 bytes stay below 2^31 bytes
  const long long HW = (long long)H * W;
  if (HW > INT_MAX / (2LL * cin) || HW > INT_MAX / (4LL * kCout * 4)) return MVN_ERR_ARG;
  const long long nTy = (H + TH - 1) / TH, nTx = (W + TW - 1) / TW;
  const long long blocks = n_images * nTy * nTx * (kCout / kBlockCout);
  if (n_images > INT_MAX || blocks > INT_MAX) return MVN_ERR_ARG;
  if (n_images == 0) return MVN_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto* xp = static_cast<const uint16_t*>(x);
  const auto* wp = static_cast<const uint4*>(weight_packed);
  const int vec = W % 4 == 0;                        // 8 outputs of a lane start on a 16-byte boundary
  if (out_layout == MVN_LAYOUT_NHWC)
    deconv4s2<false, uint16_t><<<int(blocks), kThreads, 0, st>>>(xp, wp, scale, shift, static_cast<uint16_t*>(out), H,
                                                                 W, cin, int(nTy), int(nTx), 0);
  else if (out_dtype == MVN_DTYPE_BF16)
    deconv4s2<true, uint16_t><<<int(blocks), kThreads, 0, st>>>(xp, wp, scale, shift, static_cast<uint16_t*>(out), H,
                                                                W, cin, int(nTy), int(nTx), vec);
  else
    deconv4s2<true, float><<<int(blocks), kThreads, 0, st>>>(xp, wp, scale, shift, static_cast<float*>(out), H, W,
                                                             cin, int(nTy), int(nTx), vec);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" size_t mvn_deconv4s2_project_weight_bytes(void) {
  using namespace mvn;
  return size_t(2) * kGroups * kPT * kWave * 16;
}

extern "C" int mvn_deconv4s2_project(const void* x, const void* weight_packed, const float* scale, const float* shift,
                                     const void* proj_packed, const float* bias, void* out, int out_dtype,
                                     int64_t n_images, int cin, int H, int W, void* stream) {
  using namespace mvn;
  if (!x || !weight_packed || !scale || !shift || !proj_packed || !bias || !out) return MVN_ERR_ARG;
  if (out_dtype != MVN_DTYPE_F32 && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (cin < kMinCin || cin > kMaxCin || cin % 32 != 0) return MVN_ERR_ARG;
  if (n_images < 0 || H < 1 || W < 1) return MVN_ERR_ARG;
  for (const void* p : {x, weight_packed, static_cast<const void*>(scale), static_cast<const void*>(shift), proj_packed,
                        static_cast<const void*>(bias), static_cast<const void*>(out)})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return MVN_ERR_ARG;
  // the guards of mvn_deconv4s2, as they stand there (the 32-channel output is the smaller image)
  const long long HW = (long long)H * W;
  if (HW > INT_MAX / (2LL * cin) || HW > INT_MAX / (4LL * kCout * 4)) return MVN_ERR_ARG;
  const long long nTy = (H + TH - 1) / TH, nTx = (W + TW - 1) / TW;
  const long long blocks = n_images * nTy * nTx;     // a block takes both channel halves
  if (n_images > INT_MAX || blocks * (kCout / kBlockCout) > INT_MAX) return MVN_ERR_ARG;
  if (n_images == 0) return MVN_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto* xp = static_cast<const uint16_t*>(x);
  const auto* wp = static_cast<const uint4*>(weight_packed);
  const auto* pp = static_cast<const uint4*>(proj_packed);
  const int vec = W % 4 == 0;                        // 8 outputs of a lane start on a 16-byte boundary
  if (out_dtype == MVN_DTYPE_BF16)
    deconv4s2_project<uint16_t><<<int(blocks), kThreads, 0, st>>>(xp, wp, scale, shift, pp, bias,
                                                                  static_cast<uint16_t*>(out), H, W, cin, int(nTy),
                                                                  int(nTx), vec);
  else
    deconv4s2_project<float><<<int(blocks), kThreads, 0, st>>>(xp, wp, scale, shift, pp, bias,
                                                               static_cast<float*>(out), H, W, cin, int(nTy), int(nTx),
                                                               vec);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}
