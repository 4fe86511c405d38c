// The volumetric model's process_features (mvn/models/triangulation.py:238-240, :345): a
// Conv2d(Cin, 32, 1) over NCHW maps, on the f32-input MFMA.
//
//   y[n][co][p] = b[co] + sum_ci w[co][ci] * x[n][ci][p]
//
// One arithmetic for all four dtype pairs: v_mfma_f32_32x32x2_f32 with A = the weight (rows = the
// 32 output channels), B = the maps (columns = 32 pixels), the bias as the C operand of the first
// instruction and K never split, which is bit for bit the chain
//   acc = b[co];  for ci = 0 .. Cin-1:  acc = fmaf(w[co][ci], x[n][ci][p], acc)
// (cdna_hip_programming.md §3, 'FP32-input MFMA').  A bf16 map is widened in registers (exact); a
// bf16 result is acc rounded to nearest-even.
//
// A wave takes 128 pixels of one image as four independent 32-pixel accumulators (different pixels,
// never halves of K).  Which pixels a lane holds is the only difference between the two load paths:
//   vector  pixel p0 + 4 (lane & 31) + j of accumulator j: one 16-byte (f32) or 8-byte (bf16) load
//           per lane and K-step feeds four MFMAs, and the four accumulators' values of one channel
//           are one 16-byte (f32) or 8-byte (bf16) store.  Needs H*W % 4 == 0 and aligned bases.
//   element pixel p0 + 32 j + (lane & 31): dword (f32) or 2-byte (bf16) loads and stores, any H*W
//           and any element-aligned base.
// The host chooses per call from the actual pointers and H*W.  Every load goes through one buffer
// resource per image (its Cin*H*W elements) with the byte offset of a pixel outside the image set to
// kOob, so no load touches a byte outside x; every store is predicated on its pixel.
#include <limits.h>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int kCout = 32;
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kSub = 4;                    // 32-pixel accumulators of a wave
constexpr int kTilePx = 32 * kSub;         // pixels of a wave's tile
constexpr int kChunk = 8;                  // K-steps (two input channels each) per register buffer
constexpr int kMinCin = 32, kMaxCin = 512;

typedef float f32x16_t __attribute__((ext_vector_type(16)));

// The kSub pixels of one channel row that a lane feeds to the MFMAs of one K-step, as loaded: the
// register buffers hold raw bits, and a bf16 pixel is widened by operand() next to its MFMA.  (Widened
// here, the conversions would wait for the loads in the load phase and expose their whole latency.)
// off: the lane's byte offsets into the image (kOob where the pixel is outside it); VEC reads off[0]
// only, and for bf16 fills r[0] and r[1] with the four pixels.
template <typename TI, bool VEC>
__device__ __forceinline__ void load_px(__amdgpu_buffer_rsrc_t rs, const uint32_t (&off)[kSub], uint32_t row,
                                        uint32_t (&r)[kSub]) {
  if constexpr (VEC && sizeof(TI) == 4) {
    const uint4 q = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off[0] + row, 0, 0));
    r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
  } else if constexpr (VEC) {
    const uint2 q = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs, off[0] + row, 0, 0));
    r[0] = q.x, r[1] = q.y, r[2] = 0u, r[3] = 0u;
  } else {
#pragma unroll
    for (int j = 0; j < kSub; ++j) {
      if constexpr (sizeof(TI) == 4)
        r[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, off[j] + row, 0, 0);
      else
        r[j] = uint16_t(__builtin_amdgcn_raw_buffer_load_b16(rs, off[j] + row, 0, 0));
    }
  }
}

// Pixel j of what load_px loaded, as the f32 B operand (a bf16 is widened exactly).
template <typename TI, bool VEC>
__device__ __forceinline__ float operand(const uint32_t (&r)[kSub], int j) {
  if constexpr (sizeof(TI) == 4) return __uint_as_float(r[j]);
  if constexpr (VEC) return bf16_of_pair(make_uint2(r[0], r[1]), j);
  return __uint_as_float(r[j] << 16);
}

// Grid: blocks of kWaves waves; wave w of block b takes the items (image, 128-pixel tile)
// b * kWaves + w, + gridDim.x * kWaves, ...  LDS: the weight as [ci][co] f32 (cin * 128 bytes), so
// that K-step s reads its A operand, w[lane & 31][2 s + (lane >> 5)], at dword 64 s + lane: one
// conflict-free ds_read_b32.
template <typename TI, typename TO, bool VEC>
__global__ __launch_bounds__(kThreads) void feature_conv(const TI* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, TO* __restrict__ out,
                                                         int cin, int HW, int tiles_per_image, int items, int wvec) {
  extern __shared__ float wl[];
  const int t = threadIdx.x;
  if (wvec) {
    // 16-byte reads of four consecutive ci of one row; the four LDS writes are conflict-free
    const int co = t & 31;
    for (int c4 = t >> 5; c4 < cin / 4; c4 += kThreads / 32) {
      const float4 q = *reinterpret_cast<const float4*>(w + size_t(co) * cin + 4 * c4);
      const int i = 4 * c4 * kCout + co;
      MVN_DASSERT(i >= 0 && i + 3 * kCout < cin * kCout);
      wl[i] = q.x, wl[i + kCout] = q.y, wl[i + 2 * kCout] = q.z, wl[i + 3 * kCout] = q.w;
    }
  } else {
    for (int i = t; i < cin * kCout; i += kThreads) wl[i] = w[size_t(i & 31) * cin + (i >> 5)];
  }
  __syncthreads();

  const int lane = t & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(t / kWave);
  const int q = lane & 31, h = lane >> 5;
  const uint32_t row2 = 2u * uint32_t(HW) * sizeof(TI);          // bytes between the rows of two K-steps
  const int nchunk = cin / (2 * kChunk);                          // even: cin is a multiple of 32

#pragma unroll 1
  for (int item = blockIdx.x * kWaves + wv; item < items; item += gridDim.x * kWaves) {
    const int n = item / tiles_per_image, p0 = (item - n * tiles_per_image) * kTilePx;
    const TI* xi = x + size_t(n) * cin * HW;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(xi, uint32_t(cin) * uint32_t(HW) * sizeof(TI));
    int px[kSub];
    uint32_t off[kSub];
#pragma unroll
    for (int j = 0; j < kSub; ++j) {
      px[j] = VEC ? p0 + 4 * q + j : p0 + 32 * j + q;
      off[j] = px[j] < HW ? (uint32_t(h) * HW + px[j]) * sizeof(TI) : kOob;
    }

    auto load_chunk = [&](int c, uint32_t (&buf)[kChunk][kSub]) {
#pragma unroll
      for (int s = 0; s < kChunk; ++s) load_px<TI, VEC>(rs, off, uint32_t(c * kChunk + s) * row2, buf[s]);
    };
    // register r of an accumulator is output channel (r & 3) + 8 (r >> 2) + 4 h of the lane's pixel.
    // The bias is read per item: hoisted out of the item loop, the four initial accumulators stay
    // live across it (64 registers, the second wave of a SIMD).
    int hb = h;
    asm volatile("" : "+v"(hb));
    f32x16_t acc[kSub];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float b = bias ? bias[(r & 3) + 8 * (r >> 2) + 4 * hb] : 0.f;
#pragma unroll
      for (int j = 0; j < kSub; ++j) acc[j][r] = b;
    }
    auto mfma_chunk = [&](int c, const uint32_t (&buf)[kChunk][kSub]) {
#pragma unroll
      for (int s = 0; s < kChunk; ++s) {
        const int i = (c * kChunk + s) * kWave + lane;
        MVN_DASSERT(i >= 0 && i < cin * kCout);
        const float a = wl[i];
#pragma unroll
        for (int j = 0; j < kSub; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, operand<TI, VEC>(buf[s], j), acc[j], 0, 0, 0);
      }
    };

    // two register buffers: the loads of 16 channels fly under the MFMAs of the 16 before them.
    // The last pair is peeled, so that no load in the loop is conditional and every wait counts
    // exactly the loads behind the one it needs.
    uint32_t bufA[kChunk][kSub], bufB[kChunk][kSub];
    load_chunk(0, bufA);
#pragma unroll 1
    for (int c = 0; c < nchunk - 2; c += 2) {
      load_chunk(c + 1, bufB);
      __builtin_amdgcn_sched_barrier(0);       // the scheduler otherwise sinks each load to its use
      mfma_chunk(c, bufA);
      __builtin_amdgcn_sched_barrier(0);
      load_chunk(c + 2, bufA);
      __builtin_amdgcn_sched_barrier(0);
      mfma_chunk(c + 1, bufB);
      __builtin_amdgcn_sched_barrier(0);
    }
    load_chunk(nchunk - 1, bufB);
    __builtin_amdgcn_sched_barrier(0);
    mfma_chunk(nchunk - 2, bufA);
    mfma_chunk(nchunk - 1, bufB);

    TO* oi = out + size_t(n) * kCout * HW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = (r & 3) + 8 * (r >> 2) + 4 * h;
      TO* o = oi + size_t(co) * HW;
      if constexpr (VEC) {
        if (px[0] >= HW) continue;
        MVN_DASSERT(px[0] + 3 < HW && px[0] % 4 == 0);
        if constexpr (sizeof(TO) == 4) {
          *reinterpret_cast<float4*>(o + px[0]) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        } else {
          *reinterpret_cast<uint2*>(o + px[0]) =
              make_uint2(pack_bf16x2(acc[0][r], acc[1][r]), pack_bf16x2(acc[2][r], acc[3][r]));
        }
      } else {
#pragma unroll
        for (int j = 0; j < kSub; ++j)
          if (px[j] < HW) store_elem<TO>(o + px[j], acc[j][r]);
      }
    }
  }
}

template <typename TI, typename TO>
int launch(const void* x, const float* w, const float* bias, void* out, int cin, int HW, int tiles, int items,
           hipStream_t st) {
  const auto xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
  // vector path: every channel row of every image starts on a 4-pixel boundary of both tensors
  const bool vec = HW % 4 == 0 && xa % (4 * sizeof(TI)) == 0 && oa % (4 * sizeof(TO)) == 0;
  const int wvec = reinterpret_cast<uintptr_t>(w) % 16 == 0;
  const int blocks = (items + kWaves - 1) / kWaves;
  const size_t lds = size_t(cin) * kCout * sizeof(float);
  const TI* xp = static_cast<const TI*>(x);
  TO* op = static_cast<TO*>(out);
  if (vec)
    feature_conv<TI, TO, true><<<blocks, kThreads, lds, st>>>(xp, w, bias, op, cin, HW, tiles, items, wvec);
  else
    feature_conv<TI, TO, false><<<blocks, kThreads, lds, st>>>(xp, w, bias, op, cin, HW, tiles, items, wvec);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

}  // namespace
}  // namespace mvn

extern "C" int mvn_feature_conv(const void* x, int x_dtype, const float* weight, const float* bias, void* out,
                                int out_dtype, int64_t n_images, int cin, int cout, int H, int W, void* stream) {
  using namespace mvn;
  if (!x || !weight || !out) return MVN_ERR_ARG;
  if (x_dtype != MVN_DTYPE_F32 && x_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (out_dtype != MVN_DTYPE_F32 && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_ARG;
  if (cout != kCout) return MVN_ERR_SHAPE;
  if (cin < kMinCin || cin > kMaxCin || cin % 32 != 0) return MVN_ERR_SHAPE;
  if (n_images < 0 || H < 0 || W < 0) return MVN_ERR_SHAPE;
  if (n_images == 0 || H == 0 || W == 0) return MVN_OK;
  // in-image byte offsets are 32-bit, and a buffer resource holds one image
  const long long HW = (long long)H * W, esz = x_dtype == MVN_DTYPE_F32 ? 4 : 2;
  if (HW > INT_MAX / (cin * esz)) return MVN_ERR_SHAPE;
  const long long tiles = (HW + kTilePx - 1) / kTilePx;
  if (n_images > INT_MAX / 2 / tiles) return MVN_ERR_SHAPE;     // items, and a wave's next item, are int
  const int items = int(n_images * tiles);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (x_dtype == MVN_DTYPE_F32)
    return out_dtype == MVN_DTYPE_F32
               ? launch<float, float>(x, weight, bias, out, cin, int(HW), int(tiles), items, st)
               : launch<float, uint16_t>(x, weight, bias, out, cin, int(HW), int(tiles), items, st);
  return out_dtype == MVN_DTYPE_F32
             ? launch<uint16_t, float>(x, weight, bias, out, cin, int(HW), int(tiles), items, st)
             : launch<uint16_t, uint16_t>(x, weight, bias, out, cin, int(HW), int(tiles), items, st);
}
