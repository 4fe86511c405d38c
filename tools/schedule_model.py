"""Schedule model of the four-view unprojection launch at the bench geometry (CPU only, design
aid; next to footprints.py): what the block -> tile order (csrc/x4_order.hpp) costs in idle
block slots at the end of the launch.

Every tile's staging chunk count and whether it needs several LDS passes come from the kernel's
box -> region rule; the launch is replayed with block i on XCD i % 8, each XCD filling 64 block
slots (32 CUs x 2 resident blocks) greedily in block order.  A block costs
(1 - d) + d * chunks / mean, times s for a multi-pass tile.  Efficiency = sum of the costs /
(8 * 64 * makespan).  The orders are the library's own (mvn_debug_x4_block_tiles), so the tool,
the tests and the kernel share one definition; simulate() takes any block -> tile array.
--blocks-per-cu 3 replays it for the 2-channel-slot shape (X4Shape<5>: 96 block slots per XCD).
    python tools/schedule_model.py [--frames 8] [--slots N] [--s 2.0] [--blocks-per-cu 2]"""
import argparse
import ctypes
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "learnable-triangulation-pytorch_amd"))
import lds_conflicts  # noqa: E402

TILE, KCAP = (4, 8, 16), 1024            # X4Shape<0>: voxel tile, chunk capacity of a pass
XCDS, SLOTS_PER_XCD = 8, 64
ORDERS = ("slab", "pairs", "centre-yz", "centre-3d")   # X4Order 0..3


def image_slots():
    """Image slots of one LDS pass of the f32 shape, as the library is built."""
    from mvn_rocm import _lib
    return _lib.load().mvn_debug_x4_image_slots(0)


def block_tiles(order, frames, ntiles):
    """tile of every block of a launch (order: 0..3, or -1 for the kernel's own)."""
    from mvn_rocm import _lib
    out = (ctypes.c_int * (frames * int(np.prod(ntiles))))()
    _lib.check(_lib.load().mvn_debug_x4_block_tiles(order, frames, *ntiles, out), "mvn_debug_x4_block_tiles")
    return np.frombuffer(out, dtype=np.int32).copy()


def tiles(fx, fy, ok, lim, tile=TILE, kcap=KCAP):
    """Per tile, in tile order (frame, x, y, z tiles): chunk total, slot total, passes (-1: a view
    alone exceeds a pass).  The rule of unproject_x4.hip: boxes of the base pixels + 1, odd row
    pitch, 4-pixel chunks from x & ~3, views appended to a pass while its slots and chunks fit."""
    B, NV, V = fx.shape[:3]
    n = [V // t for t in tile]
    shp = (B, NV, n[0], tile[0], n[1], tile[1], n[2], tile[2])
    big = np.iinfo(np.int64).max

    def red(a, fill, f):
        return f(np.where(ok, a, fill).reshape(shp), axis=(3, 5, 7)).reshape(B, NV, -1)
    x0, x1, y0, y1 = red(fx, big, np.min), red(fx, -big, np.max), red(fy, big, np.min), red(fy, -big, np.max)
    some = x0 <= x1
    bw, bh = np.where(some, x1 - x0 + 2, 0), np.where(some, y1 - y0 + 2, 0)
    x0 = np.where(some, x0, 0)
    area = (bw | 1) * bh
    nch = np.where(some, (x0 + bw - (x0 & ~3) + 3) >> 2, 0) * bh
    sn, cn, npass = (np.zeros(area[:, 0].shape, np.int64) for _ in range(3))
    for v in range(NV):
        new = (sn + area[:, v] > lim) | (cn + nch[:, v] > kcap)
        npass, sn, cn = npass + new, np.where(new, 0, sn) + area[:, v], np.where(new, 0, cn) + nch[:, v]
    too_big = ((area > lim) | (nch > kcap)).any(1)
    return nch.sum(1).ravel(), area.sum(1).ravel(), np.where(too_big, -1, npass + 1).ravel()


def costs(chunks, passes, d, s):
    return ((1 - d) + d * chunks / chunks.mean()) * np.where(passes == 1, 1.0, s)


def simulate(tile_of_block, cost, pooled=False):
    """Makespan and efficiency of a launch; pooled: one pool of all slots (a ticket order's bound)."""
    ends = []
    for j in range(1 if pooled else XCDS):
        slots = [0.0] * (SLOTS_PER_XCD * (XCDS if pooled else 1))
        for t in tile_of_block[j::1 if pooled else XCDS]:
            heapq.heapreplace(slots, slots[0] + cost[t])
        ends.append(max(slots))
    return max(ends), cost.sum() / (XCDS * SLOTS_PER_XCD * max(ends))


def longest_first(tile_of_block, cost, nf):
    """The same tiles per XCD and frame, the costliest first: the bound of any order within them."""
    out = tile_of_block.copy()
    for f in range(len(out) // nf):
        for j in range(XCDS):
            sel = slice(f * nf + j, (f + 1) * nf, XCDS)
            out[sel] = sorted(out[sel], key=lambda t: -cost[t])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--slots", type=int, default=0, help="image slots of a pass (default: the library's)")
    ap.add_argument("--s", type=float, default=2.0, help="cost of a multi-pass tile in one-pass tiles")
    ap.add_argument("--blocks-per-cu", type=int, default=2, help="resident blocks per CU (32 CUs per XCD)")
    a = ap.parse_args()
    global SLOTS_PER_XCD
    SLOTS_PER_XCD = 32 * a.blocks_per_cu
    lim = a.slots or image_slots()
    fx, fy, ok = lds_conflicts.geometry(B=a.frames)
    chunks, slots, passes = tiles(fx, fy, ok, lim)
    ntiles = [fx.shape[2] // t for t in TILE]
    nf = int(np.prod(ntiles))
    print(f"{len(chunks)} tiles, {lim} image slots: chunks mean {chunks.mean():.0f} sd {chunks.std():.0f} "
          f"range {chunks.min()}..{chunks.max()}; largest footprint {slots.max()} slots; "
          f"multi-pass tiles {(passes != 1).sum()} (by frame {(passes.reshape(-1, nf) != 1).sum(1).tolist()})")
    by = chunks.reshape(a.frames, ntiles[0], -1)
    print("mean chunks by x-tile:", " ".join(f"{v:.0f}" for v in by.mean((0, 2))))
    print("mean chunks by frame: ", " ".join(f"{v:.0f}" for v in by.mean((1, 2))))
    print(f"\n{'order':34s} efficiency at d = 0.3 / 0.5, and makespan against 'slab'")
    orders = [block_tiles(k, a.frames, ntiles) for k in range(len(ORDERS))]
    cost = {d: costs(chunks, passes, d, a.s) for d in (0.3, 0.5)}
    rows = [(name, {d: simulate(o, cost[d]) for d in cost}) for name, o in zip(ORDERS, orders)]
    rows.append(("pairs, longest first (bound)",
                 {d: simulate(longest_first(orders[1], cost[d], nf), cost[d]) for d in cost}))
    rows.append(("one pool, slab order (ticket bound)", {d: simulate(orders[0], cost[d], pooled=True) for d in cost}))
    for name, res in rows:
        print(f"{name:36s}" + "   ".join(f"{eff:.3f} ({100 * (mk / rows[0][1][d][0] - 1):+.1f} %)" for d, (mk, eff) in res.items()))


if __name__ == "__main__":
    main()
