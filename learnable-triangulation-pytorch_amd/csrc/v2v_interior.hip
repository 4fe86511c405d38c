// The first pooled level of the V2V's encoder-decoder (32^3 at V = 64) and its two boundaries on
// kernels for gfx950, eval mode, channels-last bf16 volumes on both sides:
//   mvn_v2v_maxpool2    encoder_pool1: F.max_pool3d(x, 2, 2), bit for bit
//   mvn_v2v_conv3_wide  the 3x3x3 conv + folded BN + skip + ReLU of the 64-channel Res3DBlocks
//                       encoder_res1 (32 -> 64), skip_res2 and decoder_res1 (64 -> 64)
//   mvn_v2v_upsample2   decoder_upsample1 (ConvTranspose3d(64, 32, 2, 2) + BN + ReLU) fused with
//                       the encoder-decoder's last `+ skip_x1`
// (mvn/models/v2v.py:20-42, 53-65, 105-135).  The arithmetic contracts are in include/mvn_hip.h.
//
// Wide conv.  v2v_res3d.hip's kernel with 64 output channels and 32 | 64 input channels: the
// same MFMA orientation (A = 16 output channels x 32 K-slots of one tap, B = 32 K-slots x 16
// z-consecutive voxels read from an LDS halo, D = 16 channels x 16 voxels), the same 4 x 8 x 16
// tile walked along x by a block of 4 waves, the same 6-slice halo ring (138,240 B at Cin = 64,
// chunk positions swizzled so that one B read covers 16 distinct bank quads).  What differs:
//   - the 27 taps' weights (110,592 | 221,184 B) do not fit beside the halo, so the A fragments
//     come straight from global memory: the packed tensor is L2-resident and a wave's fragment is
//     1 KB contiguous.  A tile is 3 dz x Cin/32 K-passes x 2 channel halves = 6 | 12 steps of 18
//     fragments (72 VGPRs); the next step's fragments are loaded into a second register set
//     under the step's 144 MFMAs, step 0's at the top of the tile;
//   - 32 accumulators per wave (8 voxel columns x 4 channel tiles, 128 registers);
//   - a column of tiles may be split into segments along x, one block each, so that 32^3 volumes
//     of a few frames still give every CU a block;
//   - the skip operands are loaded in the epilogue, when the staging registers are dead, and the
//     epilogue's per-channel constants and pointwise-skip fragments wait in LDS, which keeps
//     every instantiation out of scratch (budget: DESIGN.md §4.13).
//
// The tile, the ring's chunk positions and the staging descriptor are v2v_halo.hpp's, shared with
// v2v_conv3; this kernel gives the descriptor an 11-bit LDS index (a slice of 128-byte voxels is
// 1440 chunks), which leaves 17 bits of offset (V <= 128).
//
// Upsample.  Per input voxel a 64 -> 8 * 32 matrix product: A = 16 rows (position, channel) x
// 32 K-slots held in registers (32 fragments, 128 VGPRs, loaded once per wave), B = the 64
// channels of 16 z-consecutive voxels read straight from global memory (no halo), D = 16 tiles
// of (position p = m >> 1, channels 16 (m & 1) + 4 g + i), one 8-byte load of the skip and one
// 8-byte store per tile.
//
// Pool.  One thread per output voxel and 8 channels: eight 16-byte loads, one 16-byte store.
#include <climits>

#include "v2v_halo.hpp"

namespace mvn {
namespace {

constexpr int CO = 64, MT = CO / 16;

template <int CIN, int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void v2v_conv3_wide(
    const uint16_t* __restrict__ in, const uint4* __restrict__ wpk, const float* __restrict__ scale,
    const float* __restrict__ shift, const uint16_t* __restrict__ skip, const uint4* __restrict__ wskip,
    const float* __restrict__ scale_s, const float* __restrict__ shift_s, uint16_t* __restrict__ out, int V,
    int segTiles) {
  using R = Ring<CIN, 11>;                                   // 11-bit LDS index, 17-bit offset: V <= 128
  constexpr int CH = R::CH, kHaloChunks = R::kHaloChunks, kStage = R::kStage;   // kStage: 12 | 23
  constexpr int KP = CIN / 32;                               // K-passes per tap
  constexpr int NS = 3 * KP * 2;                             // steps per tile: (dz, K-pass, channel half)
  constexpr int kWChunks = NTAP * KP * MT * kWave;           // 16-byte chunks of the packed weights
  __shared__ uint4 halo[kHaloChunks];                        // ring of HX x-slices: [slot][hy][hz][chunk]
  __shared__ __attribute__((aligned(16))) float tab[4][CO];  // scale, shift, skip scale, skip shift
  __shared__ uint4 wsl[MT * kWave];                          // POINTWISE: the skip's A fragments [m][lane]
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(t / kWave);
  const int nTz = V / TZ, nTy = V / TY, nTx = V / TX, nSeg = nTx / segTiles;
  // blocks: (frame, ty, tz, segment), XCD-contiguous; each walks its segTiles tiles along x
  int L = xcd_remap(blockIdx.x, gridDim.x);
  const int seg = L % nSeg; L /= nSeg;
  const int tz = L % nTz; L /= nTz;
  const int ty = L % nTy; L /= nTy;
  const int b = L;
  const int y0 = ty * TY, z0 = tz * TZ, tx0 = seg * segTiles;
  const size_t nvox = size_t(V) * V * V;
  // one frame per resource: a tap outside the volume reads zero, never the neighbouring frame
  const __amdgpu_buffer_rsrc_t irs = make_rsrc(in + size_t(b) * nvox * CIN, uint32_t(nvox * CIN * 2));

  auto ld_chunk = [&](uint32_t off) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(irs, off, 0, 0));
  };
  {  // the first tile's 6 slices gx = 4 tx0 - 1 .. 4 tx0 + 4
    constexpr int kBatch = 6;
    const int gx0 = tx0 * TX - 1;
    for (int i0 = 0; i0 * kThreads < kHaloChunks; i0 += kBatch) {
      uint4 vals[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) vals[u] = ld_chunk(R::chunk_src(gx0, t + (i0 + u) * kThreads, kHaloChunks, y0, z0, V));
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int q = t + (i0 + u) * kThreads;
        MVN_DASSERT(q >= kHaloChunks || (R::chunk_dst(gx0, q) >= 0 && R::chunk_dst(gx0, q) < kHaloChunks));
        if (q < kHaloChunks) halo[R::chunk_dst(gx0, q)] = vals[u];
      }
    }
  }

  // Per-tile staging of chunk q = t + u * kThreads (u < kStage) of the 4 new slices: the
  // in-slice part is tile-invariant and decoded once into a packed descriptor
  uint32_t sdesc[kStage];
#pragma unroll
  for (int u = 0; u < kStage; ++u) sdesc[u] = R::describe1(t + u * kThreads, y0, z0, V);

  const int c = lane & 15, g = lane >> 4;
  // byte offset, within a slot, of the lane's B chunk of halo row 2 w at z offset dz, K-pass kp
  uint32_t lo[3][KP];
#pragma unroll
  for (int dz = 0; dz < 3; ++dz)
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const int hz = c + dz;
      lo[dz][kp] = uint32_t(((w * kRows * HZ + hz) * CH + chunk_pos<CH>(4 * kp + g, hz)) * 16);
    }
  // the epilogue's per-channel constants and pointwise-skip fragments wait in LDS: in registers
  // they would be live through the MFMA loop, which has none to spare
  if (t < CO) {
    tab[0][t] = scale[t];
    tab[1][t] = shift[t];
    if constexpr (MODE == MVN_SKIP_POINTWISE) {
      tab[2][t] = scale_s[t];
      tab[3][t] = shift_s[t];
    }
  }
  if constexpr (MODE == MVN_SKIP_POINTWISE) wsl[t] = wskip[t];
  const char* hbase = reinterpret_cast<const char*>(halo);
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(wpk, uint32_t(kWChunks * 16));

  // step s = (dz * KP + kp) * 2 + mh: the 9 (dx, dy) taps' A fragments of K-pass kp for the
  // channel tiles 2 mh, 2 mh + 1, from [tap][kp][m][lane]
  auto ldA = [&](uint4 (&A)[3][3][2], int s) {
    const int dz = s / (2 * KP), kp = (s >> 1) % KP, mh = s & 1;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int ml = 0; ml < 2; ++ml) {
          const int ai = ((((dx * 3 + dy) * 3 + dz) * KP + kp) * MT + 2 * mh + ml) * kWave + lane;
          MVN_DASSERT(ai >= 0 && ai < kWChunks);
          // one resource, the lane's offset in a VGPR and the fragment's in the scalar offset:
          // per-fragment 64-bit addresses, hoisted out of the tile loop, would fill the registers
          A[dx][dy][ml] = __builtin_bit_cast(
              uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane * 16, (ai - lane) * 16, 0));
        }
  };

  for (int tx = tx0; tx < tx0 + segTiles; ++tx) {
    uint4 A[2][3][3][2];
    ldA(A[0], 0);
    __syncthreads();                          // the tile's slices are in LDS
    const int x0 = tx * TX;
    const bool more = tx + 1 < tx0 + segTiles;
    const int gxn = x0 + TX + 1;              // next tile's new slices: gx = x0 + 5 .. x0 + 8
    // in flight under the MFMAs: the next tile's 4 new slices
    uint4 sv[kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) sv[u] = ld_chunk(more ? R::stage_src(sdesc[u], gxn, V) : kOob);
    // voxel (x0 + x, y0 + 2 w + yl, z0 + c) of the frame
    auto vox = [&](int x, int yl) { return ((size_t(b) * V + (x0 + x)) * V + (y0 + w * kRows + yl)) * V + z0 + c; };

    uint32_t sb[HX];                          // slot of halo x index hx (gx = x0 - 1 + hx), bytes
    const int s0 = x0 % HX;
#pragma unroll
    for (int hx = 0; hx < HX; ++hx) sb[hx] = R::slot_bytes(s0, hx);
    f32x4_t acc[TX][kRows][MT];
#pragma unroll
    for (int x = 0; x < TX; ++x)
#pragma unroll
      for (int yl = 0; yl < kRows; ++yl)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[x][yl][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // Per step: the next step's A fragments into the other register set (step 0's were loaded
    // at the top of the tile: held across the epilogue they would not fit), then the 6 x 4 halo
    // columns (hx, hyl) at z offset dz; output (x, yl) takes tap (dx, dy) from column
    // (x + dx, yl + dy).  Consecutive MFMAs go to different accumulators.
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int dz = s / (2 * KP), kp = (s >> 1) % KP, mh = s & 1;
      __builtin_amdgcn_sched_barrier(0);      // no load moves across steps: hoisted, they outgrow the register file
      if (s + 1 < NS) ldA(A[(s + 1) & 1], s + 1);
#pragma unroll
      for (int hx = 0; hx < HX; ++hx)
#pragma unroll
        for (int hyl = 0; hyl < kRows + 2; ++hyl) {
          const uint32_t off = sb[hx] + uint32_t(hyl * HZ * CH * 16) + lo[dz][kp];
          MVN_DASSERT(off + 16 <= uint32_t(kHaloChunks * 16));
          const uint4 Bv = *reinterpret_cast<const uint4*>(hbase + off);
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int x = hx - dx;
            if (x < 0 || x >= TX) continue;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
              const int yl = hyl - dy;
              if (yl < 0 || yl >= kRows) continue;
#pragma unroll
              for (int ml = 0; ml < 2; ++ml)
                acc[x][yl][2 * mh + ml] = mfma(A[s & 1][dx][dy][ml], Bv, acc[x][yl][2 * mh + ml]);
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
    uint4 As[MT];
    f32x4_t sc[MT], sh[MT], scs[MT], shs[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      sc[m] = *reinterpret_cast<const f32x4_t*>(&tab[0][16 * m + 4 * g]);
      sh[m] = *reinterpret_cast<const f32x4_t*>(&tab[1][16 * m + 4 * g]);
      if constexpr (MODE == MVN_SKIP_POINTWISE) {
        As[m] = wsl[m * kWave + lane];
        scs[m] = *reinterpret_cast<const f32x4_t*>(&tab[2][16 * m + 4 * g]);
        shs[m] = *reinterpret_cast<const f32x4_t*>(&tab[3][16 * m + 4 * g]);
      }
    }
#pragma unroll
    for (int x = 0; x < TX; ++x) {
      uint2 sk[kRows][MT];                    // IDENTITY: the lane's 4 x 4 skip channels
      uint4 skb[kRows];                       // POINTWISE: the lane's B chunk of the skip voxel
#pragma unroll
      for (int yl = 0; yl < kRows; ++yl) {
        if constexpr (MODE == MVN_SKIP_IDENTITY) {
#pragma unroll
          for (int m = 0; m < MT; ++m)
            sk[yl][m] = *reinterpret_cast<const uint2*>(skip + vox(x, yl) * CO + 16 * m + 4 * g);
        } else if constexpr (MODE == MVN_SKIP_POINTWISE) {
          skb[yl] = *reinterpret_cast<const uint4*>(skip + vox(x, yl) * 32 + 8 * g);
        }
      }
#pragma unroll
      for (int yl = 0; yl < kRows; ++yl) {
        f32x4_t accs[MT];
        if constexpr (MODE == MVN_SKIP_POINTWISE) {
          const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int m = 0; m < MT; ++m) accs[m] = mfma(As[m], skb[yl], z);
        }
        const size_t v = vox(x, yl);
        MVN_DASSERT(v < size_t(gridDim.x / (nTy * nTz * nSeg)) * nvox);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          float y[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            y[i] = bn_skip_relu<MODE>(acc[x][yl][m], sc[m], sh[m], sk[yl][m], accs[m], scs[m], shs[m], i);
          *reinterpret_cast<uint2*>(out + v * CO + 16 * m + 4 * g) = pack_bf16x4(y);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------- upsample
constexpr int UP_CI = 64, UP_CO = 32, UP_M = 16;             // 16 row tiles: (position, channel half)
constexpr int kUpChunks = 2 * UP_M * kWave;                  // [kp][m][lane]
constexpr int kUpMaxBlocks = 512;

template <bool SKIP>
__global__ __launch_bounds__(kThreads) void v2v_upsample2(const uint16_t* __restrict__ in,
                                                          const uint4* __restrict__ wpk,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const uint16_t* __restrict__ skip,
                                                          uint16_t* __restrict__ out, int V, long long ngroups) {
  const int lane = threadIdx.x & (kWave - 1), c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  uint4 A[2][UP_M];
#pragma unroll
  for (int kp = 0; kp < 2; ++kp)
#pragma unroll
    for (int m = 0; m < UP_M; ++m) {
      MVN_DASSERT((kp * UP_M + m) * kWave + lane < kUpChunks);
      A[kp][m] = wpk[(kp * UP_M + m) * kWave + lane];
    }
  float sc[2][4], sh[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[h][i] = scale[16 * h + 4 * g + i];
      sh[h][i] = shift[16 * h + 4 * g + i];
    }
  const int nz = V / 16, V2 = 2 * V;
  // one group = 16 z-consecutive input voxels; waves stride over the groups
  for (long long grp = (long long)blockIdx.x * kWaves + w; grp < ngroups; grp += (long long)gridDim.x * kWaves) {
    long long r = grp;
    const int zt = int(r % nz); r /= nz;
    const int y = int(r % V); r /= V;
    const int x = int(r % V);
    const size_t b = size_t(r / V);
    const int z = zt * 16 + c;
    const size_t iv = ((b * V + x) * V + y) * V + z;
    MVN_DASSERT(iv < size_t(ngroups) * 16);
    const uint4 B0 = *reinterpret_cast<const uint4*>(in + iv * UP_CI + 8 * g);
    const uint4 B1 = *reinterpret_cast<const uint4*>(in + iv * UP_CI + 32 + 8 * g);
#pragma unroll
    for (int m = 0; m < UP_M; ++m) {
      const int p = m >> 1, h = m & 1;                       // p = (dx * 2 + dy) * 2 + dz
      const size_t ov = ((b * V2 + 2 * x + (p >> 2)) * V2 + 2 * y + ((p >> 1) & 1)) * V2 + 2 * z + (p & 1);
      MVN_DASSERT(ov < size_t(ngroups) * 128);
      const size_t o = ov * UP_CO + 16 * h + 4 * g;
      uint2 sk = make_uint2(0u, 0u);
      if constexpr (SKIP) sk = *reinterpret_cast<const uint2*>(skip + o);
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      acc = mfma(A[0][m], B0, acc);
      acc = mfma(A[1][m], B1, acc);
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = bn_relu_add<SKIP>(acc, sc[h], sh[h], sk, i);
      *reinterpret_cast<uint2*>(out + o) = pack_bf16x4(y);
    }
  }
}

// ---------------------------------------------------------------------------- pool
// torch's max_pool3d update (v > m || isnan(v), m starting at -inf) on the bf16 bits; returns
// the winner's bits.
__device__ __forceinline__ void pool_update(uint32_t v, uint32_t& m) {
  const float fv = __uint_as_float(v << 16), fm = __uint_as_float(m << 16);
  if (fv > fm || fv != fv) m = v;
}

__global__ __launch_bounds__(kThreads) void v2v_maxpool2(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                         int V, int C8, size_t total) {
  const size_t idx = size_t(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int Vo = V / 2;
  size_t r = idx;
  const int ch = int(r % C8); r /= C8;
  const int z = int(r % Vo); r /= Vo;
  const int y = int(r % Vo); r /= Vo;
  const int x = int(r % Vo);
  const size_t b = r / Vo;
  uint32_t m[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = 0xff80u;                // -inf
#pragma unroll
  for (int dx = 0; dx < 2; ++dx)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dz = 0; dz < 2; ++dz) {
        const size_t iv = ((b * V + 2 * x + dx) * V + 2 * y + dy) * V + 2 * z + dz;
        MVN_DASSERT(iv * C8 + ch < total * 8);
        const uint4 q = in[iv * C8 + ch];
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pool_update(d[k] & 0xffffu, m[2 * k]);
          pool_update(d[k] >> 16, m[2 * k + 1]);
        }
      }
  out[idx] = make_uint4(m[0] | (m[1] << 16), m[2] | (m[3] << 16), m[4] | (m[5] << 16), m[6] | (m[7] << 16));
}

// ---------------------------------------------------------------------------- host
bool wide_volume_ok(int V) { return V >= 16 && V <= 128 && V % 16 == 0; }

// Tiles per block along x: the whole column, halved while the grid has fewer than one block per
// CU (256) and the halves stay whole and at least 2 tiles long.
int segment_tiles(int B, int V) {
  int seg = V / TX;
  long long blocks = (long long)B * (V / TY) * (V / TZ);
  while (blocks < 256 && seg % 2 == 0 && seg > 2) {
    seg /= 2;
    blocks *= 2;
  }
  return seg;
}

template <int CIN>
int launch_wide(const void* x, const void* wpk, const float* scale, const float* shift, int skip_mode,
                const void* skip, const void* wskip, const float* scale_s, const float* shift_s, void* out, int B,
                int V, hipStream_t st) {
  const int seg = segment_tiles(B, V);
  const int nblk = B * (V / TY) * (V / TZ) * ((V / TX) / seg);
  const auto* in = static_cast<const uint16_t*>(x);
  const auto* wp = static_cast<const uint4*>(wpk);
  const auto* sk = static_cast<const uint16_t*>(skip);
  const auto* ws = static_cast<const uint4*>(wskip);
  auto* o = static_cast<uint16_t*>(out);
  with_skip_mode(skip_mode, [&](auto mode) {
    v2v_conv3_wide<CIN, decltype(mode)::value><<<nblk, kThreads, 0, st>>>(in, wp, scale, shift, sk, ws, scale_s, shift_s, o, V, seg);
  });
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_v2v_conv3_wide_packed_weight_bytes(int cin) {
  return cin == 32 || cin == 64 ? size_t(mvn::NTAP) * (cin / 32) * mvn::MT * mvn::kWave * 16 : 0;
}

extern "C" size_t mvn_v2v_conv3_wide_skip_packed_weight_bytes(int cin) {
  return cin == 32 ? size_t(mvn::MT) * mvn::kWave * 16 : 0;
}

extern "C" int mvn_v2v_conv3_wide(const void* x, int cin, const void* weight_packed, const float* scale,
                                  const float* shift, int skip_mode, const void* skip, int skip_cin,
                                  const void* skip_weight_packed, const float* skip_scale,
                                  const float* skip_shift, void* out, int B, int V, void* stream) {
  using namespace mvn;
  const int rc = check_conv3_pointers(x, weight_packed, scale, shift, skip_mode, skip, skip_weight_packed, skip_scale,
                                      skip_shift, out);
  if (rc != MVN_OK) return rc;
  if (B < 1 || !wide_volume_ok(V) || (cin != 32 && cin != 64)) return MVN_ERR_SHAPE;
  if (skip_mode == MVN_SKIP_IDENTITY && skip_cin != 64) return MVN_ERR_SHAPE;
  if (skip_mode == MVN_SKIP_POINTWISE && skip_cin != 32) return MVN_ERR_SHAPE;
  if ((long long)B * (V / TY) * (V / TZ) * (V / TX) > INT_MAX) return MVN_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return cin == 32 ? launch_wide<32>(x, weight_packed, scale, shift, skip_mode, skip, skip_weight_packed, skip_scale,
                                     skip_shift, out, B, V, st)
                   : launch_wide<64>(x, weight_packed, scale, shift, skip_mode, skip, skip_weight_packed, skip_scale,
                                     skip_shift, out, B, V, st);
}

extern "C" size_t mvn_v2v_upsample2_packed_weight_bytes(void) { return size_t(mvn::kUpChunks) * 16; }

extern "C" int mvn_v2v_upsample2(const void* x, const void* weight_packed, const float* scale, const float* shift,
                                 const void* skip, void* out, int B, int V, void* stream) {
  using namespace mvn;
  if (!x || !weight_packed || !scale || !shift || !out) return MVN_ERR_ARG;
  if (B < 1 || !wide_volume_ok(V)) return MVN_ERR_SHAPE;
  const long long ngroups = (long long)B * V * V * (V / 16);
  if (ngroups > INT_MAX) return MVN_ERR_SHAPE;
  const long long want = (ngroups + kWaves - 1) / kWaves;
  const int nblk = int(want < kUpMaxBlocks ? want : kUpMaxBlocks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto* in = static_cast<const uint16_t*>(x);
  const auto* wp = static_cast<const uint4*>(weight_packed);
  auto* o = static_cast<uint16_t*>(out);
  if (skip)
    v2v_upsample2<true><<<nblk, kThreads, 0, st>>>(in, wp, scale, shift, static_cast<const uint16_t*>(skip), o, V, ngroups);
  else
    v2v_upsample2<false><<<nblk, kThreads, 0, st>>>(in, wp, scale, shift, nullptr, o, V, ngroups);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" int mvn_v2v_maxpool2(const void* x, void* out, int B, int V, int C, void* stream) {
  using namespace mvn;
  if (!x || !out) return MVN_ERR_ARG;
  if (B < 1 || V < 2 || V > 256 || V % 2 != 0 || C < 8 || C > 128 || C % 8 != 0) return MVN_ERR_SHAPE;
  const size_t Vo = size_t(V / 2), total = size_t(B) * Vo * Vo * Vo * (C / 8);
  const size_t nblk = (total + kThreads - 1) / kThreads;
  if (nblk > size_t(INT_MAX)) return MVN_ERR_SHAPE;
  v2v_maxpool2<<<int(nblk), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint4*>(x), static_cast<uint4*>(out), V, C / 8, total);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}
