// The halo ring of the tiled 3x3x3 convolutions (v2v_conv3 in v2v_res3d.hip, v2v_conv3_wide in
// v2v_interior.hip): the 4 x 8 x 16 output tile, its 6 x 10 x 18-voxel input halo kept in LDS as a
// ring of 6 x-slices (slice gx sits in slot (gx + 1) mod 6), the swizzled position of a 16-byte
// channel chunk inside a slice, and the packed descriptor of the per-tile staging.
//
// Every helper returns one value and takes its arguments by value.  The loops over a thread's
// chunks, the register arrays (sdesc, sv, sb), the buffer loads and the LDS stores stay in the
// kernels: helpers that take those arrays by reference are optimised before they are inlined and
// cost v2v_conv3<16, *> up to 16 VGPRs.  In this form the two kernels' machine code differs from
// the written-out one only in the once-per-block prologue.
#pragma once

#include "mfma.hpp"

namespace mvn {

constexpr int NTAP = 27;
constexpr int TX = 4, TY = 8, TZ = 16;
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;                 // 6, 10, 18
constexpr int kWaves = 4, kThreads = kWaves * kWave;
constexpr int kRows = TY / kWaves;                                   // output y-rows per wave: 2

// LDS position of 16-byte channel chunk c of a halo voxel at halo z index hz.  Two chunks (Cin =
// 16): the 16 z-consecutive voxels of one B read are 512 contiguous bytes, conflict-free as they
// are.  Four chunks (64-byte voxels): v2v_front's swizzle, which spreads the 16 voxels x 4 chunks
// over 16 distinct bank quads in every ds_read_b128 lane group.  Eight chunks (128-byte voxels):
// voxel pairs rotate through the 8 positions, so the 16 voxels of one B read (same chunk, any
// start) fall on 16 distinct 16-byte slots of the 256-byte bank row.
template <int CH>
__device__ __forceinline__ int chunk_pos(int c, int hz) {
  static_assert(CH == 2 || CH == 4 || CH == 8, "16, 32 or 64 input channels");
  return CH == 4 ? (c ^ (((hz >> 2) & 1) << 1)) : CH == 8 ? (c ^ ((hz >> 1) & 7)) : c;
}

// The ring of a kernel with CIN input channels whose staging descriptor gives LI_BITS bits to the
// LDS index within a slot.  Chunk q of a run of slices counts [slice][hy][hz][chunk].
//
// Staging descriptor of chunk q of the 4 new slices of a tile (the in-slice part is
// tile-invariant): bit 0 valid (q in range), bits 1-2 slice, LI_BITS bits of LDS index within the
// slot from bit 3, then one bit y/z inside the volume, the rest (gy * V + gz) * CH + c.
// LI_BITS = 10 leaves 18 bits (V <= 256 at CH <= 4), LI_BITS = 11 leaves 17 (V <= 128 at CH <= 8).
template <int CIN, int LI_BITS>
struct Ring {
  static constexpr int CH = CIN / 8;                         // 16-byte chunks per voxel record
  static constexpr int kSliceChunks = HY * HZ * CH;          // 360 | 720 | 1440 chunks per x-slice
  static constexpr int kSlotBytes = kSliceChunks * 16;       // 5,760 | 11,520 | 23,040 B
  static constexpr int kHaloChunks = HX * kSliceChunks;
  static constexpr int kStage = (TX * kSliceChunks + kThreads - 1) / kThreads;   // new-slice chunks per thread: 6 | 12 | 23
  static constexpr int kLiShift = 3, kYzShift = kLiShift + LI_BITS, kOffShift = kYzShift + 1;
  static constexpr int kOffBits = 32 - kOffShift;
  static constexpr uint32_t kLiMask = (1u << LI_BITS) - 1u, kLive = (1u << kYzShift) | 1u;
  static_assert(kSliceChunks <= (1 << LI_BITS), "the staging descriptor's LDS index does not hold a slice");

  // global byte offset, within the frame, of halo chunk q of the slices gx0, gx0 + 1, ... of the
  // tile column at (y0, z0); kOob (the load returns zero) outside the volume or past `total`
  static __device__ __forceinline__ uint32_t chunk_src(int gx0, int q, int total, int y0, int z0, int V) {
    const int sl = q / kSliceChunks, rem = q - sl * kSliceChunks;
    const int v = rem / CH, c = rem % CH;
    const int hz = v % HZ, hy = v / HZ;
    const int gx = gx0 + sl, gy = y0 + hy - 1, gz = z0 + hz - 1;
    const bool ok = (q < total) & (unsigned(gx) < unsigned(V)) & (unsigned(gy) < unsigned(V)) &
                    (unsigned(gz) < unsigned(V));
    return ok ? uint32_t(((size_t(gx) * V + gy) * V + gz) * CIN * 2 + c * 16) : kOob;
  }

  // its LDS index in the ring (gx0 >= -1 - HX)
  static __device__ __forceinline__ int chunk_dst(int gx0, int q) {
    const int sl = q / kSliceChunks, rem = q - sl * kSliceChunks;
    const int v = rem / CH, c = rem % CH;
    return ((gx0 + sl + 1 + HX) % HX) * kSliceChunks + v * CH + chunk_pos<CH>(c, v % HZ);
  }

  // the staging descriptor of chunk q
  static __device__ __forceinline__ uint32_t describe1(int q, int y0, int z0, int V) {
    const int sl = q / kSliceChunks, rem = q - sl * kSliceChunks;
    const int v = rem / CH, c = rem % CH;
    const int hz = v % HZ, hy = v / HZ;
    const int gy = y0 + hy - 1, gz = z0 + hz - 1;
    const bool valid = q < TX * kSliceChunks;
    const bool yz = (unsigned(gy) < unsigned(V)) & (unsigned(gz) < unsigned(V));
    const int li = v * CH + chunk_pos<CH>(c, hz);
    MVN_DASSERT(!valid || (sl >= 0 && sl < TX && li >= 0 && li < kSliceChunks));
    MVN_DASSERT(!yz || uint32_t((gy * V + gz) * CH + c) < (1u << kOffBits));
    return (valid ? 1u : 0u) | (uint32_t(sl & 3) << 1) | (uint32_t(li) << kLiShift) |
           (yz ? (1u << kYzShift) | (uint32_t((gy * V + gz) * CH + c) << kOffShift) : 0u);
  }

  // global byte offset of the chunk described by d in the slices gx0 .. gx0 + 3 (kOob: zero)
  static __device__ __forceinline__ uint32_t stage_src(uint32_t d, int gx0, int V) {
    const int gx = gx0 + int((d >> 1) & 3u);
    const bool ok = ((d & kLive) == kLive) & (unsigned(gx) < unsigned(V));
    return ok ? uint32_t(gx) * uint32_t(V * V * CIN * 2) + (d >> kOffShift) * 16u : kOob;
  }

  // LDS index in the ring of the valid chunk described by d, sn the slot of the first new slice
  // ((gxn + 1) mod HX, taken by the kernel: with the remainder in here v2v_conv3's POINTWISE
  // instantiations come out with two instructions of the tile loop exchanged)
  static __device__ __forceinline__ int stage_dst(uint32_t d, int sn) {
    int slot = sn + int((d >> 1) & 3u);
    if (slot >= HX) slot -= HX;
    const int li = slot * kSliceChunks + int((d >> kLiShift) & kLiMask);
    MVN_DASSERT(li >= 0 && li < kHaloChunks);
    return li;
  }

  // byte offset of the slot of halo x index hx (gx = x0 - 1 + hx) of the tile at x0, s0 = x0 mod HX
  static __device__ __forceinline__ uint32_t slot_bytes(int s0, int hx) {
    const int slot = s0 + hx >= HX ? s0 + hx - HX : s0 + hx;
    MVN_DASSERT(slot >= 0 && slot < HX);
    return uint32_t(slot * kSlotBytes);
  }
};

}  // namespace mvn
