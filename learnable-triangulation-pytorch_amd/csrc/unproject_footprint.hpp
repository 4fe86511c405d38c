// The footprint prologue of the pixel-staged unprojection kernels, unproject_tiled (forward) and
// unproject_bwd_tiled (backward): footprint_base, wave_box, layout_regions (thread 0), load_regions
// (SGPR copy), tap_slot, slot_region / slot_pixel and bilinear4.  Helpers take and return values; a
// kernel's register arrays, the loops over them and the LDS arrays stay in the kernel (DESIGN.md
// §4.1, "The shared footprint").  unproject_x4 uses none of these: its f2 weights, butterfly and
// packed RegionSet are deliberate (profiles/refactor_unproject_footprint.txt).
#pragma once

#include "unproject_common.hpp"

namespace mvn {
namespace unproj {

// Base pixel (north-west tap) and the four bilinear weights (nw, ne, sw, se) of a voxel-view.
// Returns whether at least one of the 4 taps lies inside the image and the voxel is in front of
// the camera; otherwise base pixel and weights stay as they are (the kernels' arrays start at zero).
__device__ __forceinline__ bool footprint_base(const Proj& p, bool act, int H, int W, int& fx, int& fy,
                                               float (&w)[4]) {
  const float fx0 = floorf(p.ix), fy0 = floorf(p.iy);
  const bool h = act & !p.invalid & (fx0 >= -1.f) & (fx0 < float(W)) & (fy0 >= -1.f) & (fy0 < float(H));
  if (h) {
    const float tx = p.ix - fx0, sx = 1.f - tx, ty = p.iy - fy0, sy = 1.f - ty;
    w[0] = sy * sx; w[1] = sy * tx; w[2] = ty * sx; w[3] = ty * tx;
    fx = int(fx0); fy = int(fy0);
  }
  return h;
}

// The sample of taps a (nw), b (ne), c (sw), d (se): the reference's op order.
__device__ __forceinline__ float bilinear4(float a, float b, float c, float d, const float (&w)[4]) {
  return __builtin_fmaf(d, w[3], __builtin_fmaf(c, w[2], __builtin_fmaf(b, w[1], a * w[0])));
}

// Wave-wide integer min (MAX: max), wave-uniform.  row_shr DPP steps (identity shifted in) leave
// each row's reduction in its lane 15; four readlanes combine the rows.
template <bool MAX>
__device__ __forceinline__ int wave_extreme(int v) {
  constexpr int kId = MAX ? INT_MIN : INT_MAX;
  auto pick = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
  v = pick(v, __builtin_amdgcn_update_dpp(kId, v, 0x111, 0xf, 0xf, false));
  v = pick(v, __builtin_amdgcn_update_dpp(kId, v, 0x112, 0xf, 0xf, false));
  v = pick(v, __builtin_amdgcn_update_dpp(kId, v, 0x114, 0xf, 0xf, false));
  v = pick(v, __builtin_amdgcn_update_dpp(kId, v, 0x118, 0xf, 0xf, false));
  return pick(pick(__builtin_amdgcn_readlane(v, 15), __builtin_amdgcn_readlane(v, 31)),
              pick(__builtin_amdgcn_readlane(v, 47), __builtin_amdgcn_readlane(v, 63)));
}
// The wave's box of base pixels (x0, x1, y0, y1; empty: x0 > x1) of one view, stored by lane 0.
__device__ __forceinline__ void wave_box(bool has, int fx, int fy, int lane, int (&out)[4]) {
  const int x0 = wave_extreme<false>(has ? fx : INT_MAX), x1 = wave_extreme<true>(has ? fx : INT_MIN);
  const int y0 = wave_extreme<false>(has ? fy : INT_MAX), y1 = wave_extreme<true>(has ? fy : INT_MIN);
  if (lane == 0) { out[0] = x0; out[1] = x1; out[2] = y0; out[3] = y1; }
}

// The block's LDS copy of the layout, declared by the kernel: int red[WAVES][NV][4], the waves'
// boxes; int region[NV][WORDS], per view x0, y0, bw, pitch, first slot (kRegionWords) and, for a
// kernel that takes several passes (kRegionWordsPasses), end slot, pass and the bits of 1 / pitch;
// int info[2], passes and slots of pass 0, both -1 when a footprint does not fit (a kernel that
// reads one of the two pays for one word).
constexpr int kRegionWords = 5, kRegionWordsPasses = 8;
// The same in scalar registers (a one-pass kernel: end and pass 0, 1 / pitch formed on loading).
template <int NV>
struct Regions {
  int x[NV], y[NV], bw[NV], pitch[NV], base[NV], end[NV], pass[NV];
  float inv[NV];      // 1 / pitch, correctly rounded
};

// Thread 0, between two barriers: the views' boxes over all waves -> regions of the LDS image.
template <int NV, int WAVES, int WORDS>
__device__ __forceinline__ void layout_regions(const int (&red)[WAVES][NV][4], int (&region)[NV][WORDS],
                                               int (&info)[2], int N, int budget, int max_passes) {
  int next = 0, pass = 0, slots0 = 0;
  bool too_big = false;
  for (int v = 0; v < NV; ++v) {
    if (v >= N) break;
    int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
    for (int q = 0; q < WAVES; ++q) {
      x0 = min(x0, red[q][v][0]); x1 = max(x1, red[q][v][1]);
      y0 = min(y0, red[q][v][2]); y1 = max(y1, red[q][v][3]);
    }
    int bw = 0, bh = 0;
    if (x0 <= x1) { bw = x1 - x0 + 2; bh = y1 - y0 + 2; }   // +1 px for the east / south taps
    const int pitch = bw | 1;                                 // odd: spreads rows over banks
    const long long area = (long long)pitch * bh;
    if (area > budget) too_big = true;
    if (next + area > budget) { ++pass; next = 0; }
    region[v][0] = x0; region[v][1] = y0; region[v][2] = bw; region[v][3] = pitch; region[v][4] = next;
    if constexpr (WORDS == kRegionWordsPasses) {
      region[v][5] = next + int(area);
      region[v][6] = pass;
      region[v][7] = int(__float_as_uint(1.f / float(pitch)));
    }
    next += int(area);
    if (pass == 0) slots0 = next;
  }
  const bool fits = !too_big && pass < max_passes;
  info[0] = fits ? pass + 1 : -1;
  info[1] = fits ? slots0 : -1;
}

// Block-uniform, so kept in SGPRs.
template <int NV, int WORDS>
__device__ __forceinline__ Regions<NV> load_regions(const int (&region)[NV][WORDS]) {
  Regions<NV> r{};
#pragma unroll
  for (int v = 0; v < NV; ++v) {      // (v >= N: words thread 0 never wrote; read and never used)
    r.x[v] = __builtin_amdgcn_readfirstlane(region[v][0]);
    r.y[v] = __builtin_amdgcn_readfirstlane(region[v][1]);
    r.bw[v] = __builtin_amdgcn_readfirstlane(region[v][2]);
    r.pitch[v] = __builtin_amdgcn_readfirstlane(region[v][3]);
    r.base[v] = __builtin_amdgcn_readfirstlane(region[v][4]);
    uint32_t inv = __float_as_uint(1.f / float(r.pitch[v]));
    if constexpr (WORDS == kRegionWordsPasses) {
      r.end[v] = __builtin_amdgcn_readfirstlane(region[v][5]);
      r.pass[v] = __builtin_amdgcn_readfirstlane(region[v][6]);
      inv = region[v][7];
    }
    r.inv[v] = __uint_as_float(__builtin_amdgcn_readfirstlane(inv));
  }
  return r;
}

// LDS slot of a voxel-view's north-west tap (east: the next slot; south: a pitch on); a voxel-view
// that samples nothing reads the zero slots.
__device__ __forceinline__ int tap_slot(bool has, int fx, int fy, int x0, int y0, int pitch, int base, int zero_slot) {
  const int slot = base + (fy - y0) * pitch + (fx - x0);
  MVN_DASSERT(!has || (fx >= x0 && fy >= y0 && fx - x0 < pitch && slot >= base && slot + pitch + 1 < zero_slot));
  return has ? slot : zero_slot;
}

// The region that slot idx of pass `pass` lies in.  A select chain: indexing the per-view arrays
// with a per-lane view number would force them into scratch memory.
struct SlotRegion {
  int v, x, y, bw, pitch, base;
  float inv;
};
template <int NV>
__device__ __forceinline__ SlotRegion slot_region(int idx, int pass, int N, const Regions<NV>& r) {
  SlotRegion q{0, r.x[0], r.y[0], r.bw[0], r.pitch[0], r.base[0], r.inv[0]};
#pragma unroll
  for (int u = 0; u < NV; ++u)
    if (u < N && r.pass[u] == pass && idx >= r.base[u])
      q = SlotRegion{u, r.x[u], r.y[u], r.bw[u], r.pitch[u], r.base[u], r.inv[u]};
  return q;
}
// The pixel it stages: view, image coordinates, and whether it is a pixel of the view's box inside
// the image (else the slot holds zero; an int: a bool member costs an instruction per decode).
// The row by the float reciprocal, exact for li < 2^22: (li + 0.5) / pitch is at least
// 0.5 / pitch from an integer, far above the product's rounding error.
struct SlotPixel {
  int view, gx, gy, in;
};
template <int NV>
__device__ __forceinline__ SlotPixel slot_pixel(int idx, int pass, int N, const Regions<NV>& r, int H, int W) {
  const SlotRegion q = slot_region<NV>(idx, pass, N, r);
  const int li = idx - q.base;
  const int py = int((float(li) + 0.5f) * q.inv);
  const int px = li - py * q.pitch;
  MVN_DASSERT(li < 0 || (px >= 0 && px < q.pitch));
  const int gx = q.x + px, gy = q.y + py;
  const bool in = (px < q.bw) & (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H);
  return SlotPixel{q.v, gx, gy, int(in)};
}

}  // namespace unproj
}  // namespace mvn
