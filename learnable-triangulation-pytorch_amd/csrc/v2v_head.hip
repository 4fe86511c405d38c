// V2V head on bf16 MFMA for gfx950: the pointwise tail of V2VModel in one kernel.
//
// Replaces back_layers[1], back_layers[2] (both Basic3DBlock(32, 32, 1): Conv3d 1x1x1,
// BatchNorm3d, ReLU) and output_layer = Conv3d(32, J, 1) of mvn/models/v2v.py:154-160 in eval
// mode.  Per voxel
//   h1 = relu(bn1(W1 x + b1)),  h2 = relu(bn2(W2 h1 + b2)),  y = W3 h2 + b3
// with BN and the conv bias folded by the host into a per-channel scale and shift.  The three
// layers chain in registers: HBM sees one read of x and one write of the J logits per voxel
// (as stock modules: three convolution launches, each a full pass over a 32-channel volume).
//
// MFMA v_mfma_f32_16x16x32_bf16, D = A B + C: A = 16 output channels x 32 inputs (weights),
// B = 32 inputs x 16 voxels, D = 16 channels x 16 voxels.  Lane l = (c = l & 15, g = l >> 4)
// holds A[row c][k = 8g + j], B[k = 8g + j][column c] (j = 0..7) and D[row 4g + i][column c]
// (i = 0..3).  A layer is two MFMAs per column tile (output channels 0-15 and 16-31), after
// which a lane holds, for voxel column c, the 8 channels 16m + 4g + i (m = 0, 1).  The next
// layer's K-slot 8g + j is DEFINED as channel kslot(8g + j) = 16 (j >> 2) + 4g + (j & 3), i.e.
// exactly those 8 values in the order (m, i): the lane's results, rounded to bf16, are its next
// B operand — no LDS and no cross-lane moves — and the host packs W2 and W3 under the same
// permutation.  Layer 1 reads x with the identity K-slots (channel 8g + j).
//
// A wave takes 64 consecutive voxels of a frame as 4 column tiles, tile t's column c being
// voxel 4c + t: a lane loads 4 consecutive voxels of a channel with one 16-byte (f32) or 8-byte
// (bf16) load and stores 4 consecutive logits of a joint with one.  When the frame's voxel
// count S is no multiple of 4 or a pointer is misaligned, loads and stores are per element.
// Channels-last input is one 16-byte load per lane per tile (8 channels of one voxel).
// Arithmetic: 2 * 32 * (64 + J) * S flop per frame (1.36 GFLOP at 64^3, J = 17): nothing
// beside the 33.5 MB (f32 x) + 17.8 MB (f32 logits) of traffic.
#include <climits>
#include <type_traits>

#include "mfma.hpp"

namespace mvn {
namespace {

constexpr int kC = 32;                       // channels of x, h1, h2
constexpr int kHeadWaves = 4, kHeadThreads = kHeadWaves * kWave;
constexpr int kHeadIter = 8;                 // 64-voxel chunks per wave
constexpr int kBlockVox = kHeadWaves * kHeadIter * kWave;          // 2048 voxels per block
constexpr int kLayerBytes = 2 * kWave * 16;  // packed weights of one layer: [m][lane][8] bf16

enum : int { kInNcdhwF32 = 0, kInNcdhwBf16 = 1, kInNdhwcBf16 = 2 };

struct Frag {                                // one B operand: 8 bf16 of one voxel column
  uint32_t d[4];
};

// The 64-voxel chunk at voxel v0 of a frame of S voxels, as loaded: tile t of the lane is voxel
// v0 + 4c + t, channels 8g .. 8g + 7.  No branches and no waits between the loads: a lane whose
// voxels lie past the frame reads the frame's last voxels instead (its columns are computed
// and never stored; MFMA columns do not mix).  VEC: S % 4 == 0 and 16-byte aligned rows, so the
// lane's 4 voxels are all inside or all outside; otherwise one load per element.
//   raw[] NCDHW f32: [4j + t] the f32 bits;  NCDHW bf16: VEC [2j + (t >> 1)] voxel pairs, else
//   [4j + t];  NDHWC: VEC [4t + q] channel pairs, else [8t + j]
template <int IN, bool VEC>
__device__ __forceinline__ void load_raw(const void* __restrict__ xf, int S, int v0, int c, int g,
                                         uint32_t (&raw)[32]) {
  const int v = v0 + 4 * c;
  const int vc = v < S - 4 ? v : S - 4;       // VEC only
  MVN_DASSERT(!VEC || (vc >= 0 && vc % 4 == 0 && vc + 3 < S));
  if constexpr (IN == kInNdhwcBf16) {
    const uint16_t* p = static_cast<const uint16_t*>(xf) + 8 * g;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if constexpr (VEC) {
        const uint4 r = *reinterpret_cast<const uint4*>(p + size_t(vc + t) * kC);
        raw[4 * t] = r.x; raw[4 * t + 1] = r.y; raw[4 * t + 2] = r.z; raw[4 * t + 3] = r.w;
      } else {
        const int vt = v + t < S ? v + t : S - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[8 * t + j] = p[size_t(vt) * kC + j];
      }
    }
  } else {
    using T = std::conditional_t<IN == kInNcdhwF32, float, uint16_t>;
    const T* p = static_cast<const T*>(xf) + size_t(8 * g) * S;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const T* row = p + size_t(j) * S;
      if constexpr (VEC && IN == kInNcdhwF32) {
        const uint4 r = *reinterpret_cast<const uint4*>(row + vc);
        raw[4 * j] = r.x; raw[4 * j + 1] = r.y; raw[4 * j + 2] = r.z; raw[4 * j + 3] = r.w;
      } else if constexpr (VEC) {
        const uint2 r = *reinterpret_cast<const uint2*>(row + vc);
        raw[2 * j] = r.x; raw[2 * j + 1] = r.y;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int vt = v + t < S ? v + t : S - 1;
          if constexpr (IN == kInNcdhwF32) raw[4 * j + t] = __float_as_uint(row[vt]);
          else raw[4 * j + t] = row[vt];
        }
      }
    }
  }
}

// raw[] -> the lane's 4 B operands (8 bf16 each).  f32 x is rounded to bf16 here (RNE); bf16 x
// passes through exactly.
template <int IN, bool VEC>
__device__ __forceinline__ void to_frags(const uint32_t (&raw)[32], Frag (&x)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (IN == kInNcdhwF32) {
        x[t].d[q] = pack_bf16x2(__uint_as_float(raw[8 * q + t]), __uint_as_float(raw[8 * q + 4 + t]));
      } else if constexpr (IN == kInNcdhwBf16 && VEC) {
        const uint32_t lo = raw[4 * q + (t >> 1)], hi = raw[4 * q + 2 + (t >> 1)];   // channels 2q, 2q + 1
        x[t].d[q] = (t & 1) ? (lo >> 16) | (hi & 0xffff0000u) : (lo & 0xffffu) | (hi << 16);
      } else if constexpr (IN == kInNcdhwBf16) {
        x[t].d[q] = raw[8 * q + t] | (raw[8 * q + 4 + t] << 16);
      } else if constexpr (VEC) {
        x[t].d[q] = raw[4 * t + q];
      } else {
        x[t].d[q] = raw[8 * t + 2 * q] | (raw[8 * t + 2 * q + 1] << 16);
      }
    }
}

// Grid: blocks of kBlockVox voxels, frame-major.  Wave w of a block takes the block's chunks
// w, w + 4, ...: the four waves of one iteration cover 256 consecutive voxels.
template <int IN, typename TO, bool VEC>
__global__ __launch_bounds__(kHeadThreads) void v2v_head(const void* __restrict__ x, const uint4* __restrict__ wpk,
                                                         const float* __restrict__ scale_shift,
                                                         const float* __restrict__ bias3, TO* __restrict__ out,
                                                         int J, int S, int blocks_per_frame) {
  using TI = std::conditional_t<IN == kInNcdhwF32, float, uint16_t>;
  const int lane = threadIdx.x & (kWave - 1), w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / blocks_per_frame, blk = blockIdx.x - b * blocks_per_frame;
  const TI* xf = static_cast<const TI*>(x) + size_t(b) * kC * S;
  TO* of = out + size_t(b) * J * S;
  const bool two = J > 16;                   // the third layer's channels 16..31 exist
  const int base = blk * kBlockVox + w * kWave;
  if (base >= S) return;                      // wave-uniform; the kernel has no barrier
  uint32_t raw[32];
  load_raw<IN, VEC>(xf, S, base, c, g, raw);

  // weights: A operands [layer][m][lane][8]; scale / shift / bias of the lane's 8 channels
  uint4 A[3][2];
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int m = 0; m < 2; ++m) A[l][m] = wpk[(l * 2 + m) * kWave + lane];
  float sc[2][2][4], sh[2][2][4], bj[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = 16 * m + 4 * g + i;
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        sc[l][m][i] = scale_shift[l * 2 * kC + ch];
        sh[l][m][i] = scale_shift[l * 2 * kC + kC + ch];
      }
      bj[m][i] = bias3[ch < J ? ch : J - 1];  // rows >= J are never stored
    }

  // acc (2 tiles of 4 channels) -> relu(acc * scale + shift) as the next B operand
  auto activate = [&](const f32x4_t (&acc)[2], int l, Frag& h) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = relu_keep_nan(__builtin_fmaf(acc[m][i], sc[l][m][i], sh[l][m][i]));
      h.d[2 * m] = pack_bf16x2(y[0], y[1]);
      h.d[2 * m + 1] = pack_bf16x2(y[2], y[3]);
    }
  };

  // every load of the prologue has landed: inside the loop the only loads in flight are the
  // next chunk's, which nothing waits for before the next iteration (vmcnt(0), other counters free)
  __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll 1
  for (int it = 0; it < kHeadIter; ++it) {
    const int v0 = base + it * kHeadWaves * kWave;
    if (v0 >= S) break;                       // wave-uniform
    Frag xc[4];
    to_frags<IN, VEC>(raw, xc);
    // the next chunk's loads fly under this one's MFMAs and stores
    const int vn = v0 + kHeadWaves * kWave;
    if (it + 1 < kHeadIter && vn < S) load_raw<IN, VEC>(xf, S, vn, c, g, raw);

    float y[2][4][4];                         // [m][i][t]: joint 16m + 4g + i, voxel v0 + 4c + t
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    // layer by layer over the 4 tiles: 8 independent MFMAs between dependent ones
    f32x4_t acc[4][2];
    Frag h[4];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t][0] = mfma(A[l][0], l == 0 ? xc[t] : h[t], zero);
        acc[t][1] = mfma(A[l][1], l == 0 ? xc[t] : h[t], zero);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) activate(acc[t], l, h[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[t][0] = mfma(A[2][0], h[t], zero);
      if (two) acc[t][1] = mfma(A[2][1], h[t], zero);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y[0][i][t] = acc[t][0][i] + bj[0][i];
        y[1][i][t] = two ? acc[t][1][i] + bj[1][i] : 0.f;
      }

    // rows J..31 of the padded third layer are never stored
    const int v = v0 + 4 * c;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * m + 4 * g + i;
        if (j >= J) continue;
        TO* o = of + size_t(j) * S + v;
        if constexpr (VEC) {
          if (v >= S) continue;
          MVN_DASSERT(v + 3 < S && j < J);
          if constexpr (sizeof(TO) == 4) {
            *reinterpret_cast<float4*>(o) = make_float4(y[m][i][0], y[m][i][1], y[m][i][2], y[m][i][3]);
          } else {
            *reinterpret_cast<uint2*>(o) =
                make_uint2(pack_bf16x2(y[m][i][0], y[m][i][1]), pack_bf16x2(y[m][i][2], y[m][i][3]));
          }
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            MVN_DASSERT(v + t >= S || size_t(j) * S + v + t < size_t(J) * S);
            if (v + t < S) store_elem<TO>(o + t, y[m][i][t]);
          }
        }
      }
  }
}

struct HeadShape {
  long long S;
  int blocks_per_frame;
  long long nblk;
};

// Argument checks shared by both entry points (before any HIP call).
int check_head(const void* x, int x_dtype, int x_layout, const void* wpk, const float* ss, const float* b3, int B,
               int J, int Vx, int Vy, int Vz, HeadShape* hs) {
  if (!x || !wpk || !ss || !b3) return MVN_ERR_ARG;
  if (x_layout != MVN_LAYOUT_NCDHW && x_layout != MVN_LAYOUT_NDHWC) return MVN_ERR_ARG;
  if (x_dtype != MVN_DTYPE_F32 && x_dtype != MVN_DTYPE_BF16) return MVN_ERR_DTYPE;
  if (x_dtype == MVN_DTYPE_F32 && x_layout == MVN_LAYOUT_NDHWC) return MVN_ERR_DTYPE;
  if (J < 1 || J > kC || B <= 0 || Vx <= 0 || Vy <= 0 || Vz <= 0) return MVN_ERR_SHAPE;
  const long long S = (long long)Vx * Vy * Vz;
  if (S > (1LL << 30)) return MVN_ERR_SHAPE;                    // voxel indices are int
  if (B > LLONG_MAX / (S * kC * 4)) return MVN_ERR_SHAPE;      // bytes of x and of the logits
  const long long bpf = (S + kBlockVox - 1) / kBlockVox;
  if (bpf * B > INT_MAX) return MVN_ERR_SHAPE;
  hs->S = S;
  hs->blocks_per_frame = int(bpf);
  hs->nblk = bpf * B;
  return MVN_OK;
}

template <int IN, typename TO>
int launch_head(const void* x, const void* wpk, const float* ss, const float* b3, void* out, int J,
                const HeadShape& hs, hipStream_t st) {
  // vector path: every channel row of every frame (S elements) starts 16-byte (f32) or 8-byte
  // (bf16) aligned; otherwise loads and stores are per element
  const bool vec = hs.S % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const auto* w = static_cast<const uint4*>(wpk);
  TO* o = static_cast<TO*>(out);
  const int n = int(hs.nblk), S = int(hs.S), bpf = hs.blocks_per_frame;
  if (vec)
    v2v_head<IN, TO, true><<<n, kHeadThreads, 0, st>>>(x, w, ss, b3, o, J, S, bpf);
  else
    v2v_head<IN, TO, false><<<n, kHeadThreads, 0, st>>>(x, w, ss, b3, o, J, S, bpf);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

int run_head(const void* x, int x_dtype, int x_layout, const void* wpk, const float* ss, const float* b3, void* out,
             int out_dtype, int J, const HeadShape& hs, hipStream_t st) {
  const bool of32 = out_dtype == MVN_DTYPE_F32;
  if (x_layout == MVN_LAYOUT_NDHWC)
    return of32 ? launch_head<kInNdhwcBf16, float>(x, wpk, ss, b3, out, J, hs, st)
                : launch_head<kInNdhwcBf16, uint16_t>(x, wpk, ss, b3, out, J, hs, st);
  if (x_dtype == MVN_DTYPE_F32)
    return of32 ? launch_head<kInNcdhwF32, float>(x, wpk, ss, b3, out, J, hs, st)
                : launch_head<kInNcdhwF32, uint16_t>(x, wpk, ss, b3, out, J, hs, st);
  return of32 ? launch_head<kInNcdhwBf16, float>(x, wpk, ss, b3, out, J, hs, st)
              : launch_head<kInNcdhwBf16, uint16_t>(x, wpk, ss, b3, out, J, hs, st);
}

constexpr long long kDefaultGroupBytes = 128LL << 20;           // half the MALL

int default_group(int J, long long S) {
  const long long g = kDefaultGroupBytes / (S * J * 4);
  return g < 1 ? 1 : int(g > 64 ? 64 : g);
}

size_t logits_bytes(int G, int J, long long S) { return (size_t(G) * J * S * 4 + 15) / 16 * 16; }

}  // namespace
}  // namespace mvn

extern "C" size_t mvn_v2v_head_packed_weight_bytes(int J) {
  return J < 1 || J > mvn::kC ? 0 : size_t(3) * mvn::kLayerBytes;
}

extern "C" int mvn_v2v_head(const void* x, int x_dtype, int x_layout, const void* weight_packed,
                            const float* scale_shift, const float* bias3, void* out, int out_dtype, int B, int J,
                            int Vx, int Vy, int Vz, void* stream) {
  using namespace mvn;
  if (!out) return MVN_ERR_ARG;
  HeadShape hs;
  const int rc = check_head(x, x_dtype, x_layout, weight_packed, scale_shift, bias3, B, J, Vx, Vy, Vz, &hs);
  if (rc != MVN_OK) return rc;
  if (out_dtype != MVN_DTYPE_F32 && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_DTYPE;
  return run_head(x, x_dtype, x_layout, weight_packed, scale_shift, bias3, out, out_dtype, J, hs,
                  static_cast<hipStream_t>(stream));
}

extern "C" size_t mvn_v2v_head_softargmax_workspace_bytes(int group_frames, int J, int Vx, int Vy, int Vz) {
  using namespace mvn;
  if (J < 1 || J > kC || Vx <= 0 || Vy <= 0 || Vz <= 0) return 0;
  const long long S = (long long)Vx * Vy * Vz;
  if (S > (1LL << 30)) return 0;
  const int G = group_frames > 0 ? group_frames : default_group(J, S);
  return logits_bytes(G, J, S) + mvn_softargmax3d_workspace_bytes(G, J, Vx, Vy, Vz);
}

extern "C" int mvn_v2v_head_softargmax(const void* x, int x_dtype, int x_layout, const void* weight_packed,
                                       const float* scale_shift, const float* bias3, const float* coords,
                                       const float* cuboids, int transfer_cmu, float multiplier, int softmax,
                                       float* out_xyz, void* out_vol, int out_dtype, void* workspace,
                                       size_t workspace_bytes, int group_frames, int B, int J, int Vx, int Vy, int Vz,
                                       void* stream) {
  using namespace mvn;
  if (!out_xyz) return MVN_ERR_ARG;
  if ((coords == nullptr) == (cuboids == nullptr)) return MVN_ERR_ARG;       // exactly one coordinate source
  if (softmax != 0 && softmax != 1) return MVN_ERR_ARG;
  if (transfer_cmu != 0 && transfer_cmu != 1) return MVN_ERR_ARG;
  HeadShape hs;
  int rc = check_head(x, x_dtype, x_layout, weight_packed, scale_shift, bias3, B, J, Vx, Vy, Vz, &hs);
  if (rc != MVN_OK) return rc;
  if (cuboids && (Vx != Vy || Vy != Vz)) return MVN_ERR_SHAPE;               // a cuboid grid is V^3
  if (out_dtype != MVN_DTYPE_F32 && out_dtype != MVN_DTYPE_BF16) return MVN_ERR_DTYPE;
  const int G = group_frames > 0 ? group_frames : default_group(J, hs.S);
  if (!workspace || workspace_bytes < mvn_v2v_head_softargmax_workspace_bytes(G, J, Vx, Vy, Vz))
    return MVN_ERR_WORKSPACE;
  // the soft-argmax writes a bf16 volume from bf16 logits only (mvn_softargmax3d): the logits
  // are bf16 when a bf16 volume is wanted, f32 otherwise
  const int ld = out_vol && out_dtype == MVN_DTYPE_BF16 ? MVN_DTYPE_BF16 : MVN_DTYPE_F32;
  const int sd = out_vol ? out_dtype : ld;          // no volume: the dtype pair must still be one the soft-argmax has
  const size_t S = size_t(hs.S), xe = x_dtype == MVN_DTYPE_F32 ? 4 : 2, oe = out_dtype == MVN_DTYPE_F32 ? 4 : 2;
  char* sa_ws = static_cast<char*>(workspace) + logits_bytes(G, J, hs.S);
  const size_t sa_bytes = mvn_softargmax3d_workspace_bytes(G, J, Vx, Vy, Vz);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int g = 0; g < B; g += G) {
    const int n = B - g < G ? B - g : G;
    HeadShape gs = hs;
    gs.nblk = (long long)hs.blocks_per_frame * n;
    rc = run_head(static_cast<const char*>(x) + size_t(g) * kC * S * xe, x_dtype, x_layout, weight_packed,
                  scale_shift, bias3, workspace, ld, J, gs, st);
    if (rc != MVN_OK) return rc;
    float* xyz = out_xyz + size_t(g) * J * 3;
    void* vol = out_vol ? static_cast<char*>(out_vol) + size_t(g) * J * S * oe : nullptr;
    rc = cuboids ? mvn_softargmax3d_cuboid(workspace, ld, (long long)J * hs.S, hs.S,
                                           cuboids + size_t(g) * MVN_CUBOID_FLOATS, transfer_cmu, multiplier, softmax,
                                           xyz, vol, sd, sa_ws, sa_bytes, n, J, Vx, stream)
                 : mvn_softargmax3d(workspace, ld, (long long)J * hs.S, hs.S, coords + size_t(g) * S * 3, multiplier,
                                    softmax, xyz, vol, sd, sa_ws, sa_bytes, n, J, Vx, Vy, Vz, stream);
    if (rc != MVN_OK) return rc;
  }
  return MVN_OK;
}
