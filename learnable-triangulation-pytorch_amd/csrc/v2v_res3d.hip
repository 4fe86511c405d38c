// Full-resolution Res3DBlocks of the V2V on bf16 MFMA for gfx950: one 3x3x3 convolution
// (stride 1, zero padding 1) with folded BatchNorm, an optional residual and ReLU per launch.
//
// Replaces, in eval mode, the two convolutions of Res3DBlock (mvn/models/v2v.py:20-42):
//   res_branch = Conv3d(cin, 32, 3, padding 1), BatchNorm3d, ReLU, Conv3d(32, 32, 3, padding 1),
//   BatchNorm3d;  skip_con = empty (cin == 32) or Conv3d(cin, 32, 1), BatchNorm3d;
//   y = relu(res_branch(x) + skip_con(x))
// as conv1 = relu(bn(conv(x))) (skip NONE) and conv2 = relu(bn(conv(h)) + skip) (skip IDENTITY
// or POINTWISE).  Volumes are channels-last bf16 on both sides: (B, V, V, V, Cin) in,
// (B, V, V, V, 32) out, the layout the next conv and the head (v2v_head.hip, NDHWC) read.
//
// Arithmetic per output voxel and channel co (include/mvn_hip.h, mvn_v2v_conv3):
//   acc = sum over taps and input channels of x * w   (bf16 operands, f32 accumulation, MFMA)
//   pre = fma(acc, scale[co], shift[co])
//   r   = pre | pre + float(skip) | pre + fma(acc_s, scale_s[co], shift_s[co])
//   y   = bf16(relu_keep_nan(r))
//
// MFMA v_mfma_f32_16x16x32_bf16 in the head's orientation: A = 16 output channels x 32 K-slots
// (the tap's weights, packed [tap][m][lane][8], read from LDS), B = 32 K-slots x 16 voxels (16
// z-consecutive voxels of the tap-shifted input, read from an LDS halo), D = 16 channels x 16
// voxels: lane (c = lane & 15, g = lane >> 4) ends with channels 16 m + 4 g + i (i = 0..3) of
// voxel column c, which is one 8-byte channels-last store per m.  Cin = 16 zero-pads K: the
// K-slots 16..31 hold zero weights and the lanes g >= 2 feed zeros (never halo data, so a
// non-finite voxel cannot meet a zero weight there).
//
// A block of 4 waves walks a column of 4 x 8 x 16 output tiles along x.  The 27 taps' weights
// (55,296 B) are loaded into LDS once per block; the 6 x 10 x 18-voxel input halo (69,120 B
// at Cin = 32, zero-filled outside the volume by the buffer resource's range check, as Conv3d's
// padding does) is a ring of 6 x-slices, 4 new slices per tile, loaded into registers under
// the tile's MFMAs and written to LDS once every wave is done with the slices they replace.
// Wave w computes the tile's output rows y = 2 w, 2 w + 1 for all 4 x: 8 voxel columns x 2
// channel halves = 16 accumulators; per dz it reads 18 A fragments and the 6 x 4 halo columns
// its outputs touch, each B fragment feeding up to 12 MFMAs (432 MFMAs on 126 ds_read_b128
// per wave and tile).
// Arithmetic: 2 * 27 * 32 * 32 * V^3 flop per frame (14.5 GFLOP at V = 64, Cin = 32).
//
// The tile, the ring's chunk positions and the staging descriptor are v2v_halo.hpp's, shared with
// v2v_conv3_wide; this kernel gives the descriptor a 10-bit LDS index, which leaves 18 bits of
// offset (V <= 256).
#include <climits>

#include "v2v_halo.hpp"

namespace mvn {
namespace {

constexpr int CO = 32;
constexpr int kWChunks = NTAP * 2 * kWave;                           // 3456 chunks of 16 B: [tap][m][lane]

template <int CIN, int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void v2v_conv3(
    const uint16_t* __restrict__ in, const uint4* __restrict__ wpk, const float* __restrict__ scale,
    const float* __restrict__ shift, const uint16_t* __restrict__ skip, const uint4* __restrict__ wskip,
    const float* __restrict__ scale_s, const float* __restrict__ shift_s, uint16_t* __restrict__ out, int V) {
  using R = Ring<CIN, 10>;                                   // 10-bit LDS index, 18-bit offset: V <= 256
  constexpr int CH = R::CH, kHaloChunks = R::kHaloChunks, kStage = R::kStage;   // kStage: 6 | 12
  __shared__ uint4 wl[kWChunks];                             // the 27 taps' A fragments
  __shared__ uint4 halo[kHaloChunks];                        // ring of HX x-slices: [slot][hy][hz][chunk]
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(t / kWave);
  const int nTz = V / TZ, nTy = V / TY, nTx = V / TX;
  // blocks: (frame, ty, tz), XCD-contiguous; each walks its column of nTx tiles along x
  int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tz = L % nTz; L /= nTz;
  const int ty = L % nTy; L /= nTy;
  const int b = L;
  const int y0 = ty * TY, z0 = tz * TZ;
  const size_t nvox = size_t(V) * V * V;
  // one frame per resource: a tap outside the volume reads zero, never the neighbouring frame
  const __amdgpu_buffer_rsrc_t irs = make_rsrc(in + size_t(b) * nvox * CIN, uint32_t(nvox * CIN * 2));

  for (int q = t; q < kWChunks; q += kThreads) wl[q] = wpk[q];

  auto ld_chunk = [&](uint32_t off) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(irs, off, 0, 0));
  };
  {  // the first tile's 6 slices gx = -1 .. 4
    constexpr int kBatch = 6;
    for (int i0 = 0; i0 * kThreads < kHaloChunks; i0 += kBatch) {
      uint4 vals[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) vals[u] = ld_chunk(R::chunk_src(-1, t + (i0 + u) * kThreads, kHaloChunks, y0, z0, V));
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int q = t + (i0 + u) * kThreads;
        MVN_DASSERT(q >= kHaloChunks || (R::chunk_dst(-1, q) >= 0 && R::chunk_dst(-1, q) < kHaloChunks));
        if (q < kHaloChunks) halo[R::chunk_dst(-1, q)] = vals[u];
      }
    }
  }

  // Per-tile staging of chunk q = t + u * kThreads (u < kStage) of the 4 new slices: the
  // in-slice part is tile-invariant and decoded once into a packed descriptor
  uint32_t sdesc[kStage];
#pragma unroll
  for (int u = 0; u < kStage; ++u) sdesc[u] = R::describe1(t + u * kThreads, y0, z0, V);

  const int c = lane & 15, g = lane >> 4;
  // byte offset, within a slot, of the lane's B chunk of halo row 2 w at z offset dz
  uint32_t lo[3];
#pragma unroll
  for (int dz = 0; dz < 3; ++dz) {
    const int hz = c + dz;
    lo[dz] = uint32_t(((w * kRows * HZ + hz) * CH + chunk_pos<CH>(g & (CH - 1), hz)) * 16);
  }
  const bool kpad = CH == 2 && g >= 2;                       // K-slots 16..31 of a Cin = 16 operand: zero
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  float sc[2][4], sh[2][4], scs[2][4], shs[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = 16 * m + 4 * g + i;
      sc[m][i] = scale[ch];
      sh[m][i] = shift[ch];
      if constexpr (MODE == MVN_SKIP_POINTWISE) {
        scs[m][i] = scale_s[ch];
        shs[m][i] = shift_s[ch];
      }
    }
  uint4 As[2];
  if constexpr (MODE == MVN_SKIP_POINTWISE) {
    As[0] = wskip[lane];
    As[1] = wskip[kWave + lane];
  }
  const char* hbase = reinterpret_cast<const char*>(halo);

  for (int tx = 0; tx < nTx; ++tx) {
    __syncthreads();                          // the weights and the tile's slices are in LDS
    const int x0 = tx * TX;
    const bool more = tx + 1 < nTx;
    const int gxn = x0 + TX + 1;              // next tile's new slices: gx = x0 + 5 .. x0 + 8
    // in flight under the MFMAs: the next tile's 4 new slices and this tile's skip operands
    uint4 sv[kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) sv[u] = ld_chunk(more ? R::stage_src(sdesc[u], gxn, V) : kOob);
    // voxel (x0 + x, y0 + 2 w + yl, z0 + c) of the frame
    auto vox = [&](int x, int yl) { return ((size_t(b) * V + (x0 + x)) * V + (y0 + w * kRows + yl)) * V + z0 + c; };
    uint2 sk[TX][kRows][2];                   // IDENTITY: the lane's 2 x 4 skip channels
    uint4 skb[TX][kRows];                     // POINTWISE: the lane's B chunk of the skip voxel
#pragma unroll
    for (int x = 0; x < TX; ++x)
#pragma unroll
      for (int yl = 0; yl < kRows; ++yl) {
        if constexpr (MODE == MVN_SKIP_IDENTITY) {
#pragma unroll
          for (int m = 0; m < 2; ++m)
            sk[x][yl][m] = *reinterpret_cast<const uint2*>(skip + vox(x, yl) * CO + 16 * m + 4 * g);
        } else if constexpr (MODE == MVN_SKIP_POINTWISE) {
          skb[x][yl] = *reinterpret_cast<const uint4*>(skip + vox(x, yl) * 16 + 8 * (g & 1));
        }
      }

    uint32_t sb[HX];                          // slot of halo x index hx (gx = x0 - 1 + hx), bytes
    const int s0 = x0 % HX;
#pragma unroll
    for (int hx = 0; hx < HX; ++hx) sb[hx] = R::slot_bytes(s0, hx);
    f32x4_t acc[TX][kRows][2];
#pragma unroll
    for (int x = 0; x < TX; ++x)
#pragma unroll
      for (int yl = 0; yl < kRows; ++yl)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[x][yl][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // Per dz: the 9 (dx, dy) taps' A fragments, then the 6 x 4 halo columns (hx, hyl) at z
    // offset dz; output (x, yl) takes tap (dx, dy) from column (x + dx, yl + dy).  Consecutive
    // MFMAs go to different accumulators.
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
      uint4 A[3][3][2];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            const int ai = (((dx * 3 + dy) * 3 + dz) * 2 + m) * kWave + lane;
            MVN_DASSERT(ai >= 0 && ai < kWChunks);
            A[dx][dy][m] = wl[ai];
          }
#pragma unroll
      for (int hx = 0; hx < HX; ++hx)
#pragma unroll
        for (int hyl = 0; hyl < kRows + 2; ++hyl) {
          const uint32_t off = sb[hx] + uint32_t(hyl * HZ * CH * 16) + lo[dz];
          MVN_DASSERT(off + 16 <= uint32_t(kHaloChunks * 16));
          uint4 Bv = *reinterpret_cast<const uint4*>(hbase + off);
          if (kpad) Bv = zero4;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int x = hx - dx;
            if (x < 0 || x >= TX) continue;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
              const int yl = hyl - dy;
              if (yl < 0 || yl >= kRows) continue;
#pragma unroll
              for (int m = 0; m < 2; ++m) acc[x][yl][m] = mfma(A[dx][dy][m], Bv, acc[x][yl][m]);
            }
          }
        }
    }

    __syncthreads();                          // every wave is done with the halo: the dead slots take the next slices
    if (more) {
#pragma unroll
      for (int u = 0; u < kStage; ++u) {
        const uint32_t d = sdesc[u];
        if (d & 1u) halo[R::stage_dst(d, (gxn + 1) % HX)] = sv[u];
      }
    }

    // ---- epilogue: folded BN, residual, ReLU (NaN kept, as F.relu), bf16, channels-last ----
#pragma unroll
    for (int x = 0; x < TX; ++x)
#pragma unroll
      for (int yl = 0; yl < kRows; ++yl) {
        f32x4_t accs[2];
        if constexpr (MODE == MVN_SKIP_POINTWISE) {
          const uint4 Bs = g >= 2 ? zero4 : skb[x][yl];
          const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
          accs[0] = mfma(As[0], Bs, z);
          accs[1] = mfma(As[1], Bs, z);
        }
        const size_t v = vox(x, yl);
        MVN_DASSERT(v < size_t(gridDim.x / (nTy * nTz)) * nvox);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          float y[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            y[i] = bn_skip_relu<MODE>(acc[x][yl][m], sc[m], sh[m], sk[x][yl][m], accs[m], scs[m], shs[m], i);
          *reinterpret_cast<uint2*>(out + v * CO + 16 * m + 4 * g) = pack_bf16x4(y);
        }
      }
  }
}

constexpr long long kDefaultGroupBytes = 128LL << 20;        // half the MALL

int default_group(int V) {
  const long long g = kDefaultGroupBytes / ((long long)V * V * V * CO * 2);
  return g < 1 ? 1 : int(g > 64 ? 64 : g);
}

bool volume_ok(int V) { return V >= 16 && V <= 256 && V % 16 == 0; }

// Argument checks of one launch (before any HIP call).
int check_conv3(const void* x, int cin, const void* wpk, const float* scale, const float* shift, int skip_mode,
                const void* skip, int skip_cin, const void* wskip, const float* scale_s, const float* shift_s,
                const void* out, int B, int V) {
  const int rc = check_conv3_pointers(x, wpk, scale, shift, skip_mode, skip, wskip, scale_s, shift_s, out);
  if (rc != MVN_OK) return rc;
  if (B < 1 || !volume_ok(V) || (cin != 16 && cin != 32)) return MVN_ERR_SHAPE;
  if (skip_mode == MVN_SKIP_IDENTITY && skip_cin != 32) return MVN_ERR_SHAPE;
  if (skip_mode == MVN_SKIP_POINTWISE && skip_cin != 16) return MVN_ERR_SHAPE;
  if ((long long)B * (V / TY) * (V / TZ) > INT_MAX) return MVN_ERR_SHAPE;
  return MVN_OK;
}

template <int CIN>
int launch_conv3(const void* x, const void* wpk, const float* scale, const float* shift, int skip_mode,
                 const void* skip, const void* wskip, const float* scale_s, const float* shift_s, void* out, int B,
                 int V, hipStream_t st) {
  const int nblk = B * (V / TY) * (V / TZ);                  // one block per tile column along x
  const auto* in = static_cast<const uint16_t*>(x);
  const auto* wp = static_cast<const uint4*>(wpk);
  const auto* sk = static_cast<const uint16_t*>(skip);
  const auto* ws = static_cast<const uint4*>(wskip);
  auto* o = static_cast<uint16_t*>(out);
  with_skip_mode(skip_mode, [&](auto mode) {
    v2v_conv3<CIN, decltype(mode)::value><<<nblk, kThreads, 0, st>>>(in, wp, scale, shift, sk, ws, scale_s, shift_s, o, V);
  });
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

int run_conv3(const void* x, int cin, const void* wpk, const float* scale, const float* shift, int skip_mode,
              const void* skip, const void* wskip, const float* scale_s, const float* shift_s, void* out, int B, int V,
              hipStream_t st) {
  return cin == 16 ? launch_conv3<16>(x, wpk, scale, shift, skip_mode, skip, wskip, scale_s, shift_s, out, B, V, st)
                   : launch_conv3<32>(x, wpk, scale, shift, skip_mode, skip, wskip, scale_s, shift_s, out, B, V, st);
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_v2v_conv3_packed_weight_bytes(int cin) {
  return cin == 16 || cin == 32 ? size_t(mvn::kWChunks) * 16 : 0;
}

extern "C" size_t mvn_v2v_conv3_skip_packed_weight_bytes(int cin) {
  return cin == 16 ? size_t(2) * mvn::kWave * 16 : 0;
}

extern "C" int mvn_v2v_conv3(const void* x, int cin, const void* weight_packed, const float* scale,
                             const float* shift, int skip_mode, const void* skip, int skip_cin,
                             const void* skip_weight_packed, const float* skip_scale, const float* skip_shift,
                             void* out, int B, int V, void* stream) {
  using namespace mvn;
  const int rc = check_conv3(x, cin, weight_packed, scale, shift, skip_mode, skip, skip_cin, skip_weight_packed,
                             skip_scale, skip_shift, out, B, V);
  if (rc != MVN_OK) return rc;
  return run_conv3(x, cin, weight_packed, scale, shift, skip_mode, skip, skip_weight_packed, skip_scale, skip_shift,
                   out, B, V, static_cast<hipStream_t>(stream));
}

extern "C" size_t mvn_v2v_res3d_workspace_bytes(int group_frames, int V) {
  using namespace mvn;
  if (!volume_ok(V)) return 0;
  const int G = group_frames > 0 ? group_frames : default_group(V);
  return size_t(G) * size_t(V) * V * V * CO * 2;
}

extern "C" int mvn_v2v_res3d(const void* x, int cin, const void* weight1_packed, const float* scale1,
                             const float* shift1, const void* weight2_packed, const float* scale2,
                             const float* shift2, int skip_mode, const void* skip_weight_packed,
                             const float* skip_scale, const float* skip_shift, void* out, void* workspace,
                             size_t workspace_bytes, int group_frames, int B, int V, void* stream) {
  using namespace mvn;
  if (!weight2_packed || !scale2 || !shift2) return MVN_ERR_ARG;
  if (skip_mode != MVN_SKIP_IDENTITY && skip_mode != MVN_SKIP_POINTWISE) return MVN_ERR_ARG;
  // conv2 reads the block's input as its skip; conv1's checks cover x, cin, B and V
  int rc = check_conv3(x, cin, weight1_packed, scale1, shift1, skip_mode, x, cin, skip_weight_packed, skip_scale,
                       skip_shift, out, B, V);
  if (rc != MVN_OK) return rc;
  const int G = group_frames > 0 ? group_frames : default_group(V);
  if (!workspace || workspace_bytes < mvn_v2v_res3d_workspace_bytes(G, V)) return MVN_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t nvox = size_t(V) * V * V;
  for (int g = 0; g < B; g += G) {
    const int n = B - g < G ? B - g : G;
    const char* xg = static_cast<const char*>(x) + size_t(g) * nvox * cin * 2;
    rc = run_conv3(xg, cin, weight1_packed, scale1, shift1, MVN_SKIP_NONE, nullptr, nullptr, nullptr, nullptr,
                   workspace, n, V, st);
    if (rc != MVN_OK) return rc;
    rc = run_conv3(workspace, CO, weight2_packed, scale2, shift2, skip_mode, xg, skip_weight_packed, skip_scale,
                   skip_shift, static_cast<char*>(out) + size_t(g) * nvox * CO * 2, n, V, st);
    if (rc != MVN_OK) return rc;
  }
  return MVN_OK;
}
