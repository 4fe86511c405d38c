"""The block -> tile orders of the chunk-staged unprojection (csrc/x4_order.hpp).  The kernel runs
the rotated slabs (XCD j takes the eighth (j + frame) % 8 of a frame's tiles when a frame has a
multiple of 8, the plain order otherwise); the paired orders (XCD j takes the sixteenths p and
p + 8, p = (j + frame) % 8, optionally the tiles nearest the volume's centre first, when a frame
has a multiple of 16 tiles and an even number of x-tiles) are the schedule model's candidates.

On the CPU, through the library's own helper (mvn_debug_x4_block_tiles), for every order and for
the kernel's: the map is a permutation, frames follow each other, and an XCD's blocks of a frame
lie in its eighth or its two sixteenths.  On the GPU: volumes of each class (a multiple of 16
tiles per frame, of 8, neither) at 1, 3 and 9 frames (the rotation wraps) into NaN-filled
outputs, bitwise against the generic tiled kernel and against the C oracle within the bars of
test_gpu_x4.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, max_rel
from oracle import capi
from test_gpu_x4_prologue import METHODS, SHAPES, _launch

ORDERS = (0, 1, 2, 3, -1)          # X4Order of x4_order.hpp; -1: the one the kernel is built with


def _ntiles(vol, tile):
    return tuple(-(-v // t) for v, t in zip(vol, tile))


def _block_tiles(order, frames, ntiles):
    from mvn_rocm import _lib
    out = (ctypes.c_int * (frames * ntiles[0] * ntiles[1] * ntiles[2]))()
    assert _lib.load().mvn_debug_x4_block_tiles(order, frames, *ntiles, out) == 0
    return np.frombuffer(out, dtype=np.int32).copy()


# tiles per frame (x, y, z): the test volumes under each shape's tile, and 64^3 under the three
GRIDS = ((4, 4, 2), (2, 4, 1), (1, 3, 1), (2, 4, 4), (4, 4, 4), (16, 8, 4), (8, 8, 8), (16, 8, 8),
         (2, 8, 1), (6, 4, 2), (3, 16, 1), (4, 3, 5))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("order", ORDERS)
def test_block_order_is_a_permutation_frame_by_frame(order, grid):
    nf = grid[0] * grid[1] * grid[2]
    for frames in (1, 3, 9):
        t = _block_tiles(order, frames, grid)
        assert np.array_equal(np.sort(t), np.arange(frames * nf))
        assert np.array_equal(t // nf, np.arange(frames * nf) // nf), "all XCDs work on one frame at a time"
        if nf % 8:
            assert np.array_equal(t, np.arange(frames * nf)), "plain order"


@pytest.mark.parametrize("grid", [g for g in GRIDS if (g[0] * g[1] * g[2]) % 8 == 0], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("order", ORDERS)
def test_an_xcd_takes_its_share_of_every_frame(order, grid):
    from mvn_rocm import _lib
    nf = grid[0] * grid[1] * grid[2]
    if order < 0:
        order_used = [k for k in range(4) if np.array_equal(_block_tiles(k, 9, grid), _block_tiles(-1, 9, grid))]
        assert order_used, "the kernel's order is none of the X4Orders"
    t = _block_tiles(order, 9, grid)
    blk = np.arange(t.size)
    xcd, frame, within = blk % 8, t // nf, t % nf
    p = (xcd + frame) % 8
    paired = nf % 16 == 0 and grid[0] % 2 == 0 and order != 0
    if order < 0:
        paired = paired and order_used[0] != 0
    if paired:
        sixteenth = within // (nf // 16)
        assert ((sixteenth == p) | (sixteenth == p + 8)).all()
        for j in range(8):        # half of the XCD's share from each
            assert (sixteenth[(xcd == j) & (frame == 0)] >= 8).sum() == nf // 16
    else:
        assert np.array_equal(within // (nf // 8), p)
        assert np.array_equal(t, frame * nf + p * (nf // 8) + (blk // 8) % (nf // 8)), "tile order within the eighth"
    assert _lib.load().mvn_debug_x4_block_tiles(4, 1, *grid, (ctypes.c_int * nf)()) == -1
    assert _lib.load().mvn_debug_x4_block_tiles(0, 1, *grid, None) == -1


def test_centre_orders_run_the_central_tiles_first():
    """64^3 under the f32 tile (16 x 8 x 4 tiles): XCD 0's blocks of frame 0 in the centre orders
    start at the yz centre of its planes and end in their corners."""
    grid, nf = (16, 8, 4), 512
    for order in (2, 3):
        t = _block_tiles(order, 1, grid)[0::8]
        ty, tz = (t // 4) % 8, t % 4
        d2 = (8 * ty + 4 - 32) ** 2 + (16 * tz + 8 - 32) ** 2       # voxels from the yz centre
        assert d2[:2].max() == d2.min() and d2[-2:].min() == d2.max()
        run = d2 if order == 2 else d2[:32]     # centre-3d: one plane after the other
        assert run[:len(run) // 2].mean() < run[len(run) // 2:].mean()


# ---- GPU: every order class computes what the generic kernel computes -----------------------------
# f32 tile 4 x 8 x 16: 32 tiles per frame (where the paired orders apply), 8 (the slab order only),
# 3 (the plain order)
VOLUMES_F32 = ((16, 32, 32), (8, 32, 16), (4, 24, 16))
FRAMES = (1, 3, 9)
HEATMAP, CHANNELS = 32, 8            # 8 channels: two groups, both LDS buffers


@functools.lru_cache(maxsize=None)
def _case(shape, vol, frames):
    from mvn_rocm import synth
    n_views = 8 if shape == "8v" else 4
    vb = synth.volumetric_batch(frames, n_views=n_views, channels=CHANNELS, heatmap=HEATMAP, volume=32,
                                seed=300 + frames)
    feat = vb.features.numpy()
    if shape == "bf16":     # values exactly representable in bf16
        feat = vb.features.to(torch.bfloat16).float().numpy()
    proj = vb.proj.numpy()
    coords = np.ascontiguousarray(vb.coords.numpy()[:, :vol[0], :vol[1], :vol[2]])
    conf = np.random.default_rng(frames).uniform(0.05, 1.0, (frames, n_views, CHANNELS)).astype(np.float32)
    refs = {m: capi.unproject(feat, proj, coords, m, conf) for m in METHODS}
    for a in (proj, coords, feat, conf) + tuple(refs.values()):
        a.setflags(write=False)
    return proj, coords, feat, conf, refs


def _check(device, shape, vol, frames, method, expect_tiles):
    assert int(np.prod(_ntiles(vol, SHAPES[shape]["tile"]))) == expect_tiles
    proj, coords, feat, conf, refs = _case(shape, vol, frames)
    F = torch.tensor(feat, device=device)
    if shape == "bf16":
        F = F.to(torch.bfloat16)
    P, X, cf = (torch.tensor(a, device=device) for a in (proj, coords, conf))
    a = _launch(F, P, X, cf, method, vol)
    b = _launch(F, P, X, cf, method, vol, generic=True)
    assert not torch.isnan(a).any(), "a voxel was not written"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = a.cpu().numpy()
    if method == "softmax":
        assert max_rel(got, refs[method]) <= 1e-5
    else:
        assert_bits_equal(got, refs[method])


@pytest.mark.gpu
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("vol,ntile", tuple(zip(VOLUMES_F32, (32, 8, 3))), ids=lambda v: str(v).replace(", ", "x"))
@pytest.mark.parametrize("method", METHODS)
def test_f32_order_classes_equal_generic_kernel_and_oracle(device, method, vol, ntile, frames):
    _check(device, "f32", vol, frames, method, ntile)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape,ntile", (("bf16", 32), ("8v", 64)))
def test_bf16_and_eight_view_shapes_on_a_multiple_of_16_tiles(device, shape, ntile, method):
    _check(device, shape, (16, 32, 32), 3, method, ntile)
