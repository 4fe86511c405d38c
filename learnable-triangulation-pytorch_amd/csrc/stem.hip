// The stem of the 2-D backbone's ResNet (mvn/models/pose_resnet.py:205-209, 294-297): Conv2d(3, 64, 7,
// stride 2, padding 3) + BatchNorm2d + ReLU + MaxPool2d(3, 2, 1), eval mode, in one launch on
// v_mfma_f32_16x16x32_bf16.  f32 or bf16 NCHW images in, bf16 channels-last out: what
// the trunk's first Bottleneck reads.  The arithmetic contract is in include/mvn_hip.h (mvn_stem).
//
// A block owns 8 x 8 pooled pixels of one image in all 64 channels.
//   1. It stages the 39 x 39 input pixels under them into LDS as bf16, the three planes interleaved
//      ([row][x][ci], kRowStride elements a row), through range-checked buffer loads: zeros outside the image.
//   2. The 17 x 17 convolution pixels of the tile (the pool's halo is recomputed) are 19 fragments of 16
//      flat pixels, dealt to the 4 waves.  The K axis is k = 24 ky + 3 kx + ci (three pad slots behind
//      the 21 of a tap row, padded to 192: 6 K-steps), so a lane's 8 K-slots are 8 consecutive elements
//      of one patch row: four 4-byte LDS reads.  The pad slots of a tap row lie on the pixel to the
//      right of the footprint: they are cleared in the operand (0 x NaN would be a NaN), as are the
//      slots past k = 168.  The 24 weight fragments of a lane stay in registers for the whole block.
//   3. Epilogue: fma with the folded BatchNorm, ReLU (NaN kept), ONE rounding to bf16, into an LDS map
//      [conv pixel][64 channels]; convolution pixels outside the Hc x Wc map are written as +0.
//   4. Pool: each thread takes 8 channels of a pooled pixel, the maximum over the 3 x 3 window of the LDS
//      map, one 16-byte store.  Every value of the map is +0, positive, +inf or a NaN, and every window
//      holds at least one pixel of the map, so the +0 of a pixel outside the map never changes a maximum
//      (torch pads with -inf), and the unsigned maximum of the bf16 bit patterns is torch's update
//      `v > m || isnan(v)`: the patterns of the non-negative values are ordered as the values, and a NaN
//      of either sign lies above +inf.  Rounding is monotone, so rounding before the maximum gives the
//      bits of rounding behind it.
#include <limits.h>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kCout = 64, kCin = 3, kTaps = 7;
constexpr int kTile = 8;                               // pooled pixels of a block along each axis
constexpr int kConv = 2 * kTile + 1;                   // 17 convolution pixels
constexpr int kPatch = 4 * kTile + 7;                  // 39 input pixels
constexpr int kConvPix = kConv * kConv;                // 289
constexpr int kFrags = (kConvPix + 15) / 16;           // 19
constexpr int kRowSlots = 24, kRealSlots = kTaps * kCin;   // K-slots of a tap row, 21 of them real
constexpr int kSteps = 6;                              // 192 / 32
constexpr int kGroups = kTaps * kRowSlots / 8;         // 21 groups of 8 K-slots hold weights
constexpr int kRowStride = 120;                        // bf16 of a patch row: 6 * 16 + 16 + 8 read at most
constexpr int kMapStride = 72;                         // bf16 of a convolution pixel in the LDS map: 144 bytes,
                                                       // a wave's 8-byte writes fall on all 64 banks in two passes
constexpr int kMT = kCout / 16;

static_assert(kRealSlots == kRowSlots - 3 && kGroups <= 4 * kSteps, "the operand mask clears elements 5 .. 7");
static_assert(kPatch * kCin <= kRowStride && 6 * (kConv - 1) + 16 + 8 <= kRowStride, "patch row");
static_assert(kRowStride % 2 == 0 && kMapStride % 8 == 0, "4-byte operand reads, 16-byte pool reads");

typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t max_u16x2(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, a),
                                                                __builtin_bit_cast(u16x2_t, b)));
}

template <typename T> __device__ __forceinline__ uint16_t load_bf16(const __amdgpu_buffer_rsrc_t rs, uint32_t off);
template <> __device__ __forceinline__ uint16_t load_bf16<float>(const __amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return f32_to_bf16(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0)));
}
template <> __device__ __forceinline__ uint16_t load_bf16<uint16_t>(const __amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void stem(const T* __restrict__ images, const uint4* __restrict__ wpk,
                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                 uint16_t* __restrict__ out, int M, int H, int W, int Hc, int Wc,
                                                 int Hp, int Wp, int tiles_y, int tiles_x) {
  __shared__ __attribute__((aligned(16))) uint16_t patch[kPatch * kRowStride];
  __shared__ __attribute__((aligned(16))) uint16_t cmap[kConvPix * kMapStride];

  const int t = threadIdx.x, lane = t & (kWave - 1), c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t / kWave);
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, n = b / tiles_y;
  MVN_DASSERT(n < M);
  const int py0 = ty * kTile, px0 = tx * kTile;       // the tile's first pooled pixel
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;     // its first convolution pixel (may be -1)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;     // its first input pixel (may be -5)

  // ---- 1. the input patch: [row][x][ci] bf16, zeros outside the image ----
  {
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(images, uint32_t(M) * uint32_t(kCin) * uint32_t(H) * uint32_t(W) * uint32_t(sizeof(T)));
    constexpr int kItems = kPatch * kCin * kPatch, kBatch = 6;
    constexpr int kRounds = (kItems + kThreads * kBatch - 1) / (kThreads * kBatch);
#pragma unroll 1
    for (int r = 0; r < kRounds; ++r) {
      uint16_t v[kBatch];
      int dst[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int idx = (r * kBatch + u) * kThreads + t;
        const int row = idx / (kCin * kPatch), rem = idx - row * (kCin * kPatch);
        const int ci = rem / kPatch, xx = rem - ci * kPatch;
        const int gy = iy0 + row, gx = ix0 + xx;
        const bool ok = (idx < kItems) & (unsigned(gy) < unsigned(H)) & (unsigned(gx) < unsigned(W));
        const uint32_t off = ok ? ((uint32_t(n * kCin + ci) * uint32_t(H) + uint32_t(gy)) * uint32_t(W) + uint32_t(gx)) * uint32_t(sizeof(T)) : kOob;
        v[u] = load_bf16<T>(rs, off);
        dst[u] = idx < kItems ? row * kRowStride + kCin * xx + ci : -1;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        if (dst[u] >= 0) {
          MVN_DASSERT(dst[u] < kPatch * kRowStride);
          patch[dst[u]] = v[u];
        }
    }
  }

  // ---- the lane's weight fragments and its K-slot groups ----
  uint4 A[kSteps][kMT];
#pragma unroll
  for (int s = 0; s < kSteps; ++s)
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) A[s][ml] = wpk[(s * kMT + ml) * kWave + lane];
  // group q = 4 s + g of 8 K-slots: tap row ky = q / 3, slots 8 (q % 3) .. + 7 of it
  int koff[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int q = 4 * s + g, ky = q / 3, part = q - 3 * ky;
    koff[s] = q < kGroups ? ky * kRowStride + 8 * part : -1;
  }

  __syncthreads();

  // ---- 2, 3. the convolution pixels, 16 at a time, and the epilogue into the LDS map ----
  const uint32_t* patch32 = reinterpret_cast<const uint32_t*>(patch);
#pragma unroll 1
  for (int f = wave; f < kFrags; f += kWaves) {
    const int p = f * 16 + c;
    const int pc = p < kConvPix ? p : kConvPix - 1;   // past the tile: a pixel again, not written
    const int cy = pc / kConv, cx = pc - cy * kConv;
    const int base = 2 * cy * kRowStride + 2 * kCin * cx;
    f32x4_t acc[kMT];
#pragma unroll
    for (int ml = 0; ml < kMT; ++ml) acc[ml] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const bool live = koff[s] >= 0;
      const int e = base + (live ? koff[s] : 0);
      MVN_DASSERT(e >= 0 && e % 2 == 0 && e + 8 <= kPatch * kRowStride);
      uint4 B;
      B.x = patch32[e / 2];
      B.y = patch32[e / 2 + 1];
      B.z = patch32[e / 2 + 2];
      B.w = patch32[e / 2 + 3];
      // slots 21 .. 23 of a tap row (elements 5 .. 7 of its third group) and the groups past the
      // seventh tap row hold no tap: the pixel operand is zero there, whatever lies in the patch
      const bool third = (4 * s + g) % 3 == 2;
      B.z = third ? (B.z & 0x0000ffffu) : B.z;
      B.w = third ? 0u : B.w;
      if (!live) B = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int ml = 0; ml < kMT; ++ml) acc[ml] = mfma(A[s][ml], B, acc[ml]);
    }
    // lane: channels 16 ml + 4 g + i of convolution pixel p
    const bool in_map = (unsigned(cy0 + cy) < unsigned(Hc)) & (unsigned(cx0 + cx) < unsigned(Wc));
    if (p < kConvPix) {
#pragma unroll
      for (int ml = 0; ml < kMT; ++ml) {
        const int co = 16 * ml + 4 * g;
        const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(scale + co);
        const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(shift + co);
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = relu_keep_nan(__builtin_fmaf(acc[ml][i], sc[i], sh[i]));
        const uint2 v = in_map ? pack_bf16x4(y) : make_uint2(0u, 0u);
        MVN_DASSERT(p * kMapStride + co + 4 <= kConvPix * kMapStride);
        *reinterpret_cast<uint2*>(cmap + p * kMapStride + co) = v;
      }
    }
  }

  __syncthreads();

  // ---- 4. the pool: 8 channels of a pooled pixel per thread ----
#pragma unroll
  for (int k = 0; k < kTile * kTile * (kCout / 8) / kThreads; ++k) {
    const int item = k * kThreads + t;
    const int pp = item / (kCout / 8), ch = (item % (kCout / 8)) * 8;
    const int qy = pp / kTile, qx = pp % kTile;
    const int py = py0 + qy, px = px0 + qx;
    if (py >= Hp || px >= Wp) continue;
    uint4 m = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int cp = (2 * qy + dy) * kConv + 2 * qx + dx;
        MVN_DASSERT(cp >= 0 && cp < kConvPix);
        const uint4 v = *reinterpret_cast<const uint4*>(cmap + cp * kMapStride + ch);
        m.x = max_u16x2(m.x, v.x);
        m.y = max_u16x2(m.y, v.y);
        m.z = max_u16x2(m.z, v.z);
        m.w = max_u16x2(m.w, v.w);
      }
    const size_t o = (size_t(n * Hp + py) * Wp + px) * kCout + ch;
    MVN_DASSERT(o + 8 <= size_t(M) * Hp * Wp * kCout);
    *reinterpret_cast<uint4*>(out + o) = m;
  }
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_stem_packed_weight_bytes(void) {
  using namespace mvn;
  return size_t(kSteps) * kMT * kWave * 16;
}

extern "C" int mvn_stem(const void* images, int in_dtype, const void* weight_packed, const float* scale,
                        const float* shift, void* out, int64_t n_images, int H, int W, void* stream) {
  using namespace mvn;
  if (!images || !weight_packed || !scale || !shift || !out) return MVN_ERR_ARG;
  if (in_dtype != MVN_DTYPE_F32 && in_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (n_images < 0 || H < 1 || W < 1) return MVN_ERR_ARG;
  const long long esize = in_dtype == MVN_DTYPE_F32 ? 4 : 2;
  const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
  // the images and the output below 2^31 bytes (the images are the larger: 3 H W esize >= 64 Hp Wp 2 / 1.4
  // does not hold for tiny maps, so both are checked)
  if (n_images > INT_MAX) return MVN_ERR_ARG;
  long long in_bytes = (long long)n_images * kCin;
  for (long long f : {(long long)H, (long long)W, esize}) {
    in_bytes *= f;
    if (in_bytes > (long long)INT_MAX) return MVN_ERR_ARG;
  }
  long long out_bytes = (long long)n_images * kCout * 2;
  for (long long f : {(long long)Hp, (long long)Wp}) {
    out_bytes *= f;
    if (out_bytes > (long long)INT_MAX) return MVN_ERR_ARG;
  }
  if (reinterpret_cast<uintptr_t>(images) % uintptr_t(esize) != 0) return MVN_ERR_ARG;
  for (const void* p : {weight_packed, static_cast<const void*>(scale), static_cast<const void*>(shift),
                        static_cast<const void*>(out)})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return MVN_ERR_ARG;
  if (n_images == 0) return MVN_OK;
  const int tiles_y = (Hp + kTile - 1) / kTile, tiles_x = (Wp + kTile - 1) / kTile;
  const long long blocks = (long long)n_images * tiles_y * tiles_x;   // below 2^31 / 128 pooled pixels
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (in_dtype == MVN_DTYPE_F32)
    stem<float><<<int(blocks), kThreads, 0, st>>>(static_cast<const float*>(images), static_cast<const uint4*>(weight_packed),
                                                  scale, shift, static_cast<uint16_t*>(out), int(n_images), H, W, Hc, Wc,
                                                  Hp, Wp, tiles_y, tiles_x);
  else
    stem<uint16_t><<<int(blocks), kThreads, 0, st>>>(static_cast<const uint16_t*>(images),
                                                     static_cast<const uint4*>(weight_packed), scale, shift,
                                                     static_cast<uint16_t*>(out), int(n_images), H, W, Hc, Wc, Hp, Wp,
                                                     tiles_y, tiles_x);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}
