// The backbone's confidence heads (mvn/models/pose_resnet.py:140-174, GlobalAveragePoolingHead), eval
// mode, in two kernels: the 3x3 convolution with its bias and BatchNorm folded, the
// 2x2 max pool and the ReLU behind it in one launch on v_mfma_f32_16x16x32_bf16 (twice per head), and
// the mean over the pixels with the three Linear layers and the Sigmoid in one launch on the vector
// ALU.  The arithmetic contracts are in include/mvn_hip.h (mvn_conv3x3_pool, mvn_confidence_tail).
//
// conv3x3_pool is bottleneck.hip's implicit GEMM (weights as A, 64 channels x 64 pixels per wave,
// operands straight from global memory through a range-checked buffer resource, the next K-step's
// loads in flight under this step's 16 MFMAs) run over pool windows instead of pixels: a 16-column
// fragment is 16 consecutive windows (n, py, px) of the whole batch, and the wave's four fragments
// j = 0..3 are the four conv pixels (2 py + (j >> 1), 2 px + (j & 1)) of those windows.  A lane then
// holds the four pixels of one window for four consecutive channels, so the pool is a maximum over j
// in registers.  An odd trailing row or column of conv pixels belongs to no window and is not computed.
//
// Parallelism.  The head's maps are small (6 x 6 windows per image behind 384 x 384 images) and K is long
// (9 Cin / 32 = 576 steps at 2048 channels), so a block is 4 waves on ONE window tile of one 64-channel
// group, with K split over them: wave s takes the K-steps [s per, (s + 1) per), per = 9 Cin / 32 / 4 rounded
// up to even, tap-major.  Waves 1..3 leave their accumulators in LDS (48 KB) and wave 0 adds them in the
// order ((a0 + a1) + a2) + a3 before the epilogue: one fixed order, deterministic, no atomics.  bottleneck.hip's
// block (4 waves on 4 consecutive tiles, each over the whole K) was measured beside this one and was slower
// on every shape of the head at 8 x 4 and 32 x 4 views, so it is not kept.
#include <limits.h>
#include <math.h>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kMT = 4, kNT = 4;                      // 16-channel tiles and the 4 pixels of a window
constexpr int kGroupC = 16 * kMT;                    // 64 output channels of a block
constexpr int kTileWin = 16;                         // windows of a wave's tile
constexpr int kMinC = 64, kMaxCin = 2048, kMaxCout = 512;

// acc[ml][j] = the sum over the K-steps it = k0 .. k1 - 1 (k1 - k0 even, possibly 0) of
// A(it, m0 + ml) x B(it, j): A from wpk as [it][m 0..mtiles-1][lane], B the 16 bytes at byte offset
// off(it, j) behind rs.  bottleneck.hip's mfma_loop over a range of steps.
template <typename OffF>
__device__ __forceinline__ void mfma_range(const __amdgpu_buffer_rsrc_t rs, const uint4* __restrict__ wpk, int mtiles,
                                           int m0, int k0, int k1, int lane, OffF off, f32x4_t (&acc)[kMT][kNT]) {
  auto load = [&](int it, uint4 (&A)[kMT], uint4 (&B)[kNT]) {
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) {
      const int ai = ((it * mtiles) + m0 + ml) * kWave + lane;
      MVN_DASSERT(it >= k0 && it < k1 && m0 + ml < mtiles && ai >= 0);
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
  if (k0 >= k1) return;                              // an empty slice of a short K (wave-uniform)

  uint4 A0[kMT], B0[kNT], A1[kMT], B1[kNT];
  load(k0, A0, B0);
#pragma unroll 1
  for (int it = k0; it < k1; it += 2) {
    load(it + 1, A1, B1);
    __builtin_amdgcn_sched_barrier(0);               // the next step's loads are requested before this step's MFMAs
    mma(A0, B0);
    __builtin_amdgcn_sched_barrier(0);
    load(it + 2 < k1 ? it + 2 : it, A0, B0);         // past the end: a step again, in bounds, unused
    __builtin_amdgcn_sched_barrier(0);
    mma(A1, B1);
  }
}

__device__ __forceinline__ void store4(uint16_t* p, const float (&y)[4]) { *reinterpret_cast<uint2*>(p) = pack_bf16x4(y); }
__device__ __forceinline__ void store4(float* p, const float (&y)[4]) {
  *reinterpret_cast<f32x4_t*>(p) = f32x4_t{y[0], y[1], y[2], y[3]};
}

template <typename OutT>
__global__ __launch_bounds__(kThreads) void conv3x3_pool(const uint16_t* __restrict__ x, const uint4* __restrict__ wpk,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         OutT* __restrict__ out, int NW, int cin, int cout, int H, int W,
                                                         int Hp, int Wp) {
  constexpr int KS = kWaves;                         // the block's waves split K
  const int lane = threadIdx.x & (kWave - 1), c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int groups = cout / kGroupC;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int cg = L % groups;
  const int tile = L / groups, ks = w;
  const int w0 = tile * kTileWin;
  MVN_DASSERT(w0 < NW);                              // one block per tile, every tile holds a window: no wave leaves early

  // the lane's window and, for its four conv pixels, the input pixel of tap (0, 0) with its flat index
  // in x (may be negative: used only where the tap is inside the image)
  const __amdgpu_buffer_rsrc_t rsx = make_rsrc(x, uint32_t(NW / (Hp * Wp)) * uint32_t(H * W) * uint32_t(cin) * 2u);
  const int wi = w0 + c;
  const bool live = wi < NW;
  int iy0[kNT], ix0[kNT], pix0[kNT];
  {
    const int q = live ? wi : 0;
    const int n = q / (Hp * Wp), rem = q - n * (Hp * Wp);
    const int py = rem / Wp, px = rem - py * Wp;
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      iy0[j] = 2 * py + (j >> 1) - 1;
      ix0[j] = 2 * px + (j & 1) - 1;
      pix0[j] = (n * H + iy0[j]) * W + ix0[j];
      MVN_DASSERT(iy0[j] + 1 < H && ix0[j] + 1 < W);
    }
  }
  const int KP = cin / 32;
  // it / KP by a float multiply, it < 576 and KP <= 64: (it + 0.5) / KP lies at least 0.5 / KP >= 2^-7 from
  // an integer and below 9; the roundings of 1 / KP and of the product move it by less than 9 * 2^-23
  const float inv_kp = 1.0f / float(KP);
  auto off = [&](int it, int j) -> uint32_t {
    const int tap = int((float(it) + 0.5f) * inv_kp);
    const int kp = it - tap * KP;
    const int ky = tap / 3, kx = tap - 3 * ky;
    MVN_DASSERT(tap >= 0 && tap < 9 && kp >= 0 && kp < KP);
    const bool ok = live & (unsigned(iy0[j] + ky) < unsigned(H)) & (unsigned(ix0[j] + kx) < unsigned(W));
    return ok ? uint32_t(pix0[j] + ky * W + kx) * (uint32_t(cin) * 2u) + 16u * g + uint32_t(kp) * 64u : kOob;
  };
  const int total = 9 * KP;                          // even: cin is a multiple of 64
  const int per = (((total + KS - 1) / KS) + 1) & ~1;
  const int k0 = min(ks * per, total), k1 = min(k0 + per, total);
  f32x4_t acc[kMT][kNT];
  mfma_range(rsx, wpk, cout / 16, cg * kMT, k0, k1, lane, off, acc);

  __shared__ f32x4_t red[KS - 1][kMT * kNT][kWave];
  if (ks > 0) {
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml)
#pragma unroll
      for (int j = 0; j < kNT; ++j) red[ks - 1][ml * kNT + j][lane] = acc[ml][j];
  }
  __syncthreads();
  if (ks > 0) return;
#pragma unroll
  for (int s = 1; s < KS; ++s)
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml)
#pragma unroll
      for (int j = 0; j < kNT; ++j) acc[ml][j] = acc[ml][j] + red[s - 1][ml * kNT + j][lane];
  if (!live) return;

  // ---- epilogue: the fold per conv pixel, the maximum over the window (torch's update: a NaN wins), the
  // ReLU (NaN kept), one rounding, one 8- or 16-byte store.  lane: channels co + i of window wi
#pragma unroll
  for (int ml = 0; ml < kMT; ++ml) {
    const int co = cg * kGroupC + 16 * ml + 4 * g;
    const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(scale + co);
    const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(shift + co);
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float m = __builtin_fmaf(acc[ml][0][i], sc[i], sh[i]);
#pragma unroll
      for (int j = 1; j < kNT; ++j) {
        const float r = __builtin_fmaf(acc[ml][j][i], sc[i], sh[i]);
        m = (r > m || r != r) ? r : m;
      }
      y[i] = relu_keep_nan(m);
    }
    store4(out + size_t(wi) * cout + co, y);
  }
}

// ---- the tail: mean over the pixels, three Linear layers, the activation; one block per image ----
constexpr int kTailThreads = 256, kTailMaxWidth = 512, kTailMaxN = 32;

// outv[o] = act(bias[o] + the fma chain over i ascending of wt[i][o] * in[i]) for the block's outputs
template <bool RELU>
__device__ __forceinline__ void tail_linear(const float* __restrict__ wt, const float* __restrict__ bias,
                                            const float* in, float* outv, int ci, int co) {
  for (int o = threadIdx.x; o < co; o += kTailThreads) {
    float acc = bias[o];
#pragma unroll 8
    for (int i = 0; i < ci; ++i) acc = __builtin_fmaf(wt[size_t(i) * co + o], in[i], acc);
    outv[o] = RELU ? relu_keep_nan(acc) : acc;
  }
}

__global__ __launch_bounds__(kTailThreads) void confidence_tail(const float* __restrict__ x,
                                                                const float* __restrict__ params,
                                                                float* __restrict__ out, int hw, int c0, int c1, int c2,
                                                                int n, int act) {
  __shared__ float a[kTailMaxWidth], b[kTailMaxWidth];
  const float* xm = x + size_t(blockIdx.x) * hw * c0;
  for (int ch = threadIdx.x; ch < c0; ch += kTailThreads) {
    float s = 0.f;
    for (int p = 0; p < hw; ++p) s = s + xm[size_t(p) * c0 + ch];
    a[ch] = s / float(hw);
  }
  __syncthreads();
  const float* w1 = params;
  const float* b1 = w1 + size_t(c0) * c1;
  const float* w2 = b1 + c1;
  const float* b2 = w2 + size_t(c1) * c2;
  const float* w3 = b2 + c2;
  const float* b3 = w3 + size_t(c2) * n;
  tail_linear<true>(w1, b1, a, b, c0, c1);
  __syncthreads();
  tail_linear<true>(w2, b2, b, a, c1, c2);
  __syncthreads();
  tail_linear<false>(w3, b3, a, b, c2, n);           // b[0 .. n - 1]: the logits, each read by its own thread
  if (int(threadIdx.x) < n) {
    const float z = b[threadIdx.x];
    out[size_t(blockIdx.x) * n + threadIdx.x] = act == MVN_ACT_SIGMOID ? 1.0f / (1.0f + expf(-z)) : z;
  }
}

inline bool channels_ok(int c, int max_c) { return c >= kMinC && c <= max_c && c % 64 == 0; }

// n_images * H * W pixels of `channels` elements of `elem` bytes below 2^31 bytes; the pixel count in *pixels.
inline bool tensor_fits(int64_t n_images, int H, int W, int channels, int elem, long long* pixels) {
  if (n_images > INT_MAX) return false;
  long long p = (long long)n_images * H;
  if (p > INT_MAX) return false;
  p *= W;
  if (p > INT_MAX || p * channels * elem > (long long)INT_MAX) return false;
  *pixels = p;
  return true;
}

template <typename OutT>
void launch_pool(const void* x, const void* wpk, const float* scale, const float* shift, void* out, long long NW,
                 int cin, int cout, int H, int W, hipStream_t st) {
  const long long blocks = ((NW + kTileWin - 1) / kTileWin) * (cout / kGroupC);     // below 2^31 / 16
  conv3x3_pool<OutT><<<int(blocks), kThreads, 0, st>>>(
      static_cast<const uint16_t*>(x), static_cast<const uint4*>(wpk), scale, shift, static_cast<OutT*>(out), int(NW),
      cin, cout, H, W, H / 2, W / 2);
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_conv3x3_pool_packed_weight_bytes(int cin, int cout) {
  using namespace mvn;
  return channels_ok(cin, kMaxCin) && channels_ok(cout, kMaxCout) ? size_t(9) * (cin / 32) * (cout / 16) * kWave * 16 : 0;
}

extern "C" int mvn_conv3x3_pool(const void* x, const void* weight_packed, const float* scale, const float* shift,
                                void* out, int out_dtype, int64_t n_images, int H, int W, int cin, int cout,
                                void* stream) {
  using namespace mvn;
  if (!x || !weight_packed || !scale || !shift || !out) return MVN_ERR_ARG;
  if (!channels_ok(cin, kMaxCin) || !channels_ok(cout, kMaxCout)) return MVN_ERR_ARG;
  if (out_dtype != MVN_DTYPE_F32 && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (n_images < 0 || H < 2 || W < 2) return MVN_ERR_ARG;
  for (const void* p : {x, weight_packed, (const void*)scale, (const void*)shift, (const void*)out})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return MVN_ERR_ARG;
  long long Pin, NW;
  if (!tensor_fits(n_images, H, W, cin, 2, &Pin) ||
      !tensor_fits(n_images, H / 2, W / 2, cout, out_dtype == MVN_DTYPE_F32 ? 4 : 2, &NW))
    return MVN_ERR_ARG;
  if (n_images == 0) return MVN_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (out_dtype == MVN_DTYPE_BF16) launch_pool<uint16_t>(x, weight_packed, scale, shift, out, NW, cin, cout, H, W, st);
  else launch_pool<float>(x, weight_packed, scale, shift, out, NW, cin, cout, H, W, st);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" size_t mvn_confidence_tail_packed_bytes(int c0, int c1, int c2, int n) {
  using namespace mvn;
  if (!channels_ok(c0, kTailMaxWidth) || !channels_ok(c1, kTailMaxWidth) || !channels_ok(c2, kTailMaxWidth) || n < 1 ||
      n > kTailMaxN)
    return 0;
  return (size_t(c0) * c1 + c1 + size_t(c1) * c2 + c2 + size_t(c2) * n + n) * sizeof(float);
}

extern "C" int mvn_confidence_tail(const float* pooled, const float* params, float* out, int64_t n_images, int hw,
                                   int c0, int c1, int c2, int n, int activation, void* stream) {
  using namespace mvn;
  if (!pooled || !params || !out) return MVN_ERR_ARG;
  if (mvn_confidence_tail_packed_bytes(c0, c1, c2, n) == 0) return MVN_ERR_ARG;
  if (activation != MVN_ACT_NONE && activation != MVN_ACT_SIGMOID) return MVN_ERR_ARG;
  if (n_images < 0 || hw < 1) return MVN_ERR_ARG;
  for (const void* p : {(const void*)pooled, (const void*)params, (const void*)out})
    if (reinterpret_cast<uintptr_t>(p) % 4 != 0) return MVN_ERR_ARG;
  long long P;
  if (!tensor_fits(n_images, hw, 1, c0, 4, &P)) return MVN_ERR_ARG;
  if (n_images == 0) return MVN_OK;
  confidence_tail<<<int(n_images), kTailThreads, 0, static_cast<hipStream_t>(stream)>>>(pooled, params, out, hw, c0, c1,
                                                                                      c2, n, activation);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}
