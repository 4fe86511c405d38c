// Block -> tile order of the chunk-staged unprojection (unproject_x4.hip): one definition for
// the kernel, the host entry mvn_debug_x4_block_tiles (debug.hip) and, through that entry,
// tools/schedule_model.py and the tests.  Scalar integer arithmetic on the block index only.
//
// Hardware deals blocks round-robin over the 8 XCDs (block i runs on XCD i % 8) and each XCD
// starts its blocks in index order, so the order decides which tiles an XCD takes and which of
// them it runs last.  Tiles are numbered frame-major, then x, y, z tiles with z fastest; a
// frame's nf tiles cut into equal runs of that numbering are runs of x-planes ("slabs").  The
// staged footprint of a tile, and with it the tile's cost, falls off with its distance from
// the volume centre (tools/schedule_model.py), for every frame alike.
//
// The kernel runs kX4OrderSlab.  The other orders are what the schedule model was built to
// compare; on the GPU they lost to it (profiles/r23_ab_variants.txt) and
// stay here as the model's and the tests' subjects only.
#pragma once

#if defined(__HIPCC__)
#define MVN_HD __host__ __device__
#else
#define MVN_HD
#endif

namespace mvn {
namespace unproj {

enum X4Order {
  kX4OrderSlab = 0,      // XCD j takes the eighth (j + frame) % 8 of a frame, in tile order
  kX4OrderPairs = 1,     // ... the sixteenths p and p + 8, p = (j + frame) % 8, in tile order
  kX4OrderCentreYZ = 2,  // ... alternating between the two, each from its yz centre outwards
  kX4OrderCentre3D = 3,  // ... the sixteenth nearer the volume's centre first, then the other
};

// Position r = 0 .. n-1 -> index in [0, n), the middle first: n/2, n/2 - 1, n/2 + 1, ...
MVN_HD inline int centre_out(int r, int n) {
  const int h = (r + 1) >> 1;
  return n / 2 + ((r & 1) ? -h : h);
}

// Tile (frame * nf + (tx * nTy + ty) * nTz + tz) of block blk.  A bijection of [0, B * nf).
//  * nf % 8 != 0: the plain order.
//  * nf % 8 == 0: all XCDs work on one frame at a time and XCD j on the slab (j + frame) % 8,
//    so over 8 frames every XCD sees every slab position (kX4OrderSlab).
//  * nf % 16 == 0 and nTx even (the other orders): XCD j takes the sixteenths p and p + 8 —
//    one from each x-half of the volume, a light outer one with a heavy inner one, which
//    evens the XCDs' totals within a frame.  The centre orders also run each XCD's heavy
//    tiles first and the light ones last, so that the 64 block slots of an XCD run dry within
//    one light tile of each other: a sixteenth of whole yz-planes is walked plane by plane,
//    each plane from its centre outwards (z rings outer, y inner); any other sixteenth from the
//    middle of its run outwards.
MVN_HD inline int x4_block_tile(int blk, int nTx, int nTy, int nTz, int order) {
  const int nf = nTx * nTy * nTz;
  if (nf % 8 != 0) return blk;
  const int xcd = blk % 8, k = blk / 8, slab = nf / 8;
  const int frame = k / slab, m = k % slab, p = (xcd + frame) % 8;
  if (order == kX4OrderSlab || nf % 16 != 0 || nTx % 2 != 0) return frame * nf + p * slab + m;
  const int g = nf / 16, plane = nTy * nTz;
  int half, r;
  if (order == kX4OrderCentreYZ) {
    half = m & 1; r = m >> 1;
  } else {
    half = m / g; r = m % g;
    if (order == kX4OrderCentre3D && p < 4) half ^= 1;    // sixteenth p + 8 is the nearer one
  }
  int i = r;
  if (order != kX4OrderPairs) {
    if (g % plane == 0) {
      const int q = r % plane;
      i = r - q + centre_out(q % nTy, nTy) * nTz + centre_out(q / nTy, nTz);
    } else {
      i = centre_out(r, g);
    }
  }
  return frame * nf + (p + 8 * half) * g + i;
}

}  // namespace unproj
}  // namespace mvn
