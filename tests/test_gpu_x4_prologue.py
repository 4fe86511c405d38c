"""The tile prologue of the chunk-staged unprojection (csrc/unproject_x4.hip): block -> tile
order (the x-slab an XCD takes rotates with the frame when a frame has a multiple of 8 tiles),
footprint boxes, LDS regions and chunk descriptors.  Small volumes whose tiles are built to hit
every descriptor case, asserted on the CPU by restating the kernel's box -> chunk-count rule:

  a. the chunk total fits the first chunk slot and leaves at least one whole wave without a chunk;
  b. the total needs more than one chunk slot per thread and still takes one pass
     (shapes with one chunk slot per thread, the bf16 tile, cannot have it);
  c. the views do not fit one LDS pass together (several passes of whole views);
  d. a view in which no voxel of the tile samples the image.

Every case compares the kernel bitwise with the generic tiled kernel and with the C oracle within
the bars of test_gpu_x4.py, on an output buffer pre-filled with NaN (an unwritten voxel shows).
MI355X only."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, max_rel
from oracle import capi

pytestmark = pytest.mark.gpu

METHODS = ("sum", "max", "softmax", "conf")
LIM = 2048 - 2 - 64          # image slots of an LDS buffer (kTrash in unproject_x4.hip)
# X4Shape of a call: voxel tile, threads per block, chunk capacity of a pass (MC * threads)
SHAPES = {
    "f32": dict(tile=(4, 8, 16), threads=512, kcap=1024),      # X4Shape<0>
    "bf16": dict(tile=(8, 8, 8), threads=512, kcap=512),       # X4Shape<2>
    "8v": dict(tile=(4, 8, 8), threads=256, kcap=768),         # X4Shape<3>
}
# Voxel spacing (mm along x, y, z at a 96-pixel heatmap; scaled by 96 / H for others, so that the
# footprints keep their size in pixels) of the four geometry classes per shape: small footprints;
# narrow tall ones (many chunks per LDS slot: more than a chunk per thread within one buffer);
# large ones; small ones moved sideways out of the cameras that look along x.  A class fills an
# 8-row y-half and a 16-voxel z-half of a frame, so every tile of every shape lies in one class.
SPACING = {
    "f32": ((18, 18, 18), (10, 10, 125), (90, 90, 90), (18, 18, 18)),
    "bf16": ((18, 18, 18), (40, 40, 40), (100, 100, 100), (18, 18, 18)),
    "8v": ((18, 18, 18), (10, 10, 80), (120, 120, 120), (18, 18, 18)),
}
CENTERS = np.array([[0.0, 0.0, 900.0], [0.0, 0.0, 900.0], [0.0, 0.0, 900.0], [0.0, 2600.0, 900.0]])


def _coords(B, vol, spacing, heatmap=96):
    """(B, Vx, Vy, Vz, 3) float32: class (b + Y // 8 + 2 * (Z // 16)) % 4 of a voxel selects the
    lattice it lies on (op.py:99 takes any coordinate volume), centred on the class's point."""
    Vx, Vy, Vz = vol
    b, X, Y, Z = np.meshgrid(np.arange(B), np.arange(Vx), np.arange(Vy), np.arange(Vz), indexing="ij")
    k = (b + Y // 8 + 2 * (Z // 16)) % 4
    local = np.stack([X - (Vx - 1) / 2.0, Y % 8 - 3.5, Z % 16 - 7.5], -1)
    return (CENTERS[k] + np.asarray(spacing, np.float64)[k] * (96.0 / heatmap) * local).astype(np.float32)


def _tiles(proj, coords, H, W, tile, threads, kcap):
    """Per tile: (chunk total of the first pass, passes or -1 for the gather fallback, a view
    without a sample) — the kernel's rule: boxes of the base pixels + 1, odd row pitch, 4-pixel
    chunks from x & ~3, views appended to a pass while its slots and chunks fit."""
    TX, TY, TZ = tile
    B, Vx, Vy, Vz = coords.shape[:4]
    X = np.concatenate([coords, np.ones(coords.shape[:4] + (1,))], -1).astype(np.float64)
    uvw = np.einsum("bvrk,bxyzk->bvxyzr", proj.astype(np.float64), X)
    w = np.where(uvw[..., 2] == 0, 1.0, uvw[..., 2])
    fx = np.floor((2 * (uvw[..., 0] / w / H - 0.5) + 1) * W / 2 - 0.5)
    fy = np.floor((2 * (uvw[..., 1] / w / W - 0.5) + 1) * H / 2 - 0.5)
    ok = (fx >= -1) & (fx < W) & (fy >= -1) & (fy < H) & (uvw[..., 2] > 0)
    out = []
    for b in range(B):
        for x in range(0, Vx, TX):
            for y in range(0, Vy, TY):
                for z in range(0, Vz, TZ):
                    snext = cnext = npass = chunks0 = 0
                    too_big = empty = False
                    for v in range(proj.shape[1]):
                        sl = (b, v, slice(x, x + TX), slice(y, y + TY), slice(z, z + TZ))
                        m = ok[sl]
                        area = nch = 0
                        if m.any():
                            x0, y0 = int(fx[sl][m].min()), int(fy[sl][m].min())
                            bw, bh = int(fx[sl][m].max()) - x0 + 2, int(fy[sl][m].max()) - y0 + 2
                            area, nch = (bw | 1) * bh, ((x0 + bw - (x0 & ~3) + 3) >> 2) * bh
                        else:
                            empty = True
                        too_big |= area > LIM or nch > kcap
                        if snext + area > LIM or cnext + nch > kcap:
                            npass, snext, cnext = npass + 1, 0, 0
                        snext, cnext = snext + area, cnext + nch
                        if npass == 0:
                            chunks0 = cnext
                    out.append((chunks0, -1 if too_big else npass + 1, empty))
    return out


def _assert_cases(tiles, threads, kcap):
    """The four descriptor cases among the tiles, with 32 chunks of margin (the kernel forms the
    boxes in f32, this model in f64: a box edge may differ by a pixel)."""
    one = [t for t in tiles if t[1] == 1]
    assert any(0 < t[0] <= threads - 64 - 32 for t in one), "no tile leaves a whole wave without a chunk"
    if kcap > threads:
        assert any(threads + 32 <= t[0] <= kcap - 32 for t in one), "no one-pass tile fills a second chunk slot"
    assert any(t[1] > 1 for t in tiles), "no multi-pass tile"
    assert any(t[2] for t in tiles), "no tile with a view that samples nothing"


@functools.lru_cache(maxsize=None)
def _case(shape, vol, frames, heatmap, channels):
    """Inputs (numpy, read-only), the tiles' cases and the oracle's outputs per aggregation."""
    from mvn_rocm import synth
    n_views = 8 if shape == "8v" else 4
    rng = np.random.default_rng(1000 * frames + vol[0])
    cams = synth.ring_cameras(n_views, rng)
    proj = np.repeat(synth.projections(cams, heatmap_size=heatmap)[None], frames, 0).astype(np.float32)
    coords = _coords(frames, vol, SPACING[shape], heatmap)
    feat = rng.standard_normal((frames, n_views, channels, heatmap, heatmap)).astype(np.float32)
    if shape == "bf16":     # values exactly representable in bf16
        feat = torch.from_numpy(feat).to(torch.bfloat16).float().numpy()
    conf = rng.uniform(0.05, 1.0, (frames, n_views, channels)).astype(np.float32)
    s = SHAPES[shape]
    tiles = _tiles(proj, coords, heatmap, heatmap, s["tile"], s["threads"], s["kcap"])
    refs = {m: capi.unproject(feat, proj, coords, m, conf) for m in METHODS}
    for a in (proj, coords, feat, conf) + tuple(refs.values()):
        a.setflags(write=False)
    return proj, coords, feat, conf, tiles, refs


def _launch(feat, proj, coords, conf, method, vol, channels_last=False, generic=False):
    """mvn_unproject(_ex) through the C ABI into a NaN-filled f32 buffer of the test's own."""
    from mvn_rocm import _lib
    lib = _lib.load()
    B, N, C, H, W = feat.shape
    Vx, Vy, Vz = vol
    out = torch.full((B, Vx, Vy, Vz, C) if channels_last else (B, C, Vx, Vy, Vz), float("nan"),
                     dtype=torch.float32, device=feat.device)
    code = _lib.MVN_DTYPE_BF16 if feat.dtype == torch.bfloat16 else _lib.MVN_DTYPE_F32
    agg = METHODS.index(method)
    assert (_lib.MVN_AGG_SUM, _lib.MVN_AGG_MAX, _lib.MVN_AGG_SOFTMAX, _lib.MVN_AGG_CONF) == (0, 1, 2, 3)
    with _lib.unproject_knobs(generic=generic):
        _lib.check(lib.mvn_unproject_ex(
            feat.data_ptr(), code, proj.data_ptr(), coords.data_ptr(), conf.data_ptr(), out.data_ptr(),
            _lib.MVN_DTYPE_F32, _lib.MVN_LAYOUT_NDHWC if channels_last else _lib.MVN_LAYOUT_NCDHW,
            B, N, C, H, W, Vx, Vy, Vz, agg, 0, torch.cuda.current_stream().cuda_stream), "mvn_unproject_ex")
        torch.cuda.synchronize()
    return out


def _check(device, shape, vol, frames, heatmap, channels, method, channels_last=False):
    proj, coords, feat, conf, tiles, refs = _case(shape, vol, frames, heatmap, channels)
    s = SHAPES[shape]
    _assert_cases(tiles, s["threads"], s["kcap"])
    F = torch.tensor(feat, device=device)
    if shape == "bf16":
        F = F.to(torch.bfloat16)
    P, X, cf = (torch.tensor(a, device=device) for a in (proj, coords, conf))
    a = _launch(F, P, X, cf, method, vol, channels_last)
    b = _launch(F, P, X, cf, method, vol, channels_last, generic=True)
    assert not torch.isnan(a).any(), "a voxel was not written"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = (a.permute(0, 4, 1, 2, 3) if channels_last else a).cpu().numpy()
    if method == "softmax":
        assert max_rel(got, refs[method]) <= 1e-5
    else:
        assert_bits_equal(np.ascontiguousarray(got), refs[method])


# volume, frames, heatmap, channels: (8, 16, 32) is 8 tiles per frame (4 x 8 x 16 and 8 x 8 x 8
# tiles alike), so the slab rotation is live; (4, 8, 16) is one f32 tile per frame and (6, 10, 20)
# has partial tiles with inactive lanes, both in the fallback block order
GEOMETRIES = (((8, 16, 32), 1, 96, 8), ((8, 16, 32), 3, 88, 4), ((8, 16, 32), 9, 96, 4),
              ((4, 8, 16), 4, 96, 8), ((6, 10, 20), 4, 88, 4))


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "v{}x{}x{}-b{}-h{}-c{}".format(*g[0], *g[1:]))
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", ("f32", "bf16"))
def test_prologue_cases_equal_generic_kernel_and_oracle(device, shape, method, geo):
    _check(device, shape, *geo, method)


@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_prologue_cases_channels_last(device, method):
    _check(device, "f32", (8, 16, 32), 3, 96, 8, method, channels_last=True)


@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_prologue_cases_eight_views(device, method):
    _check(device, "8v", (8, 16, 32), 3, 96, 4, method)
