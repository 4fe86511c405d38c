"""The fast unprojection's range guards, and the fast kernels no other test launches (MI355X only).

precision='fast' computes the view softmax without its max pass; a denominator outside
[2^-100, 2^120] sends the work back to a max-first form (csrc/unproject_x4.hip):
  deferred guard   4 views with bf16 maps, or f32 maps written NCDHW: the range over all channel
                   groups is checked once per wave after the channel loop, and a tripping wave
                   rewrites every channel of its voxels with the exact gather_voxel
  per-group guard  8 views, or 4 views of f32 maps written channels-last: each channel group
                   checks its own range and redoes itself max-first

Every reference is the pinned C oracle (oracle.capi.unproject) on the same f32 arrays / bf16 bits.

Bars.  Only the joints' 1e-4 is north_star's (BASELINE.json); the volume bars are this project's
own, written in tests/test_gpu_fast.py's docstring and used here unchanged:
  f32 maps            max-rel <= 1e-4
  bf16 maps, f32 out  max-rel <= 2^-7 for softmax (2^-8 otherwise)
  bf16 maps, bf16 out one bf16 ulp of the oracle + the f32-out bar x max|ref|
max-rel divides by max|ref|, which is ~100 in a channel block that carries an offset and ~3 in one
that does not, so the guard tests apply a bar per frame and, in the offset frame, per 4-channel
block: a wrong in-range block cannot hide behind a neighbour's magnitude.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import max_rel
from oracle import capi
from test_gpu_fast import F32_TOL, METHODS, assert_bf16_fast, bf16_bar, bf16_bits
from test_gpu_parity import tile_footprints

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
DEN_HI, DEN_LO = 2.0 ** 120, 2.0 ** -100          # the guards' thresholds (unproject_x4.hip)
RAGGED = (13, 21, 10)                             # a corner of a 24^3 volume: partial tiles on every axis


def _bits(t):
    return bf16_bits(t) if t.dtype == torch.bfloat16 else t.numpy()


def _oracle(feat, proj, coords, method="softmax", **kw):
    return capi.unproject(_bits(feat), np.asarray(proj), np.asarray(coords), method,
                          feat_bf16_bits=feat.dtype == torch.bfloat16, **kw)


def channel_classes(channels, cycle=(0, 1, 2, 3)):
    """Class of each channel: blocks of 4 consecutive channels, the class cycling with the block."""
    return np.asarray(cycle)[(np.arange(channels) // 4) % len(cycle)]


@functools.lru_cache(maxsize=None)
def guard_inputs(n_views, channels, volume, seed, dtype, crop=None, cuboid=False, cycle=(0, 1, 2, 3)):
    """Two frames of unit-variance maps (synth.volumetric_batch, 64^2 maps).  Frame 0 is left as it
    is; frame 1 gets a per-view constant added to each block of 4 channels, by the block's class:
      0  nothing                                             in range
      1  odd views +U(88, 110) (view 1: +100), even views -U(88, 110)   some denominator > 2^120
      2  every view -U(75, 100)                                denominator < 2^-100 where every view samples
      3  every view U(-72, +84)                                inside the range on both sides
    The offsets come from np.random.default_rng(seed).  No device is needed: the builder checks on
    the CPU, from the oracle's per-view samples (each view unprojected alone with 'sum'), that the
    float64 denominators den = sum_v 2^(s_v log2 e) fall where the classes say, and raises
    otherwise (change the seed then, not the thresholds).  The result is cached and read-only.

    ``crop``: (x, y, z) extents cut from the coordinate volume's corner (a ragged volume).
    ``cuboid``: the coordinates are oracle.restate_np.coord_volumes of the frames' cuboids (what
    volumetric.build_cuboids forms in-kernel) instead of synth's torch-built volume; the two agree
    to an ulp, not on every host bit for bit.
    ``cycle``: the classes the blocks cycle through (all four by default)."""
    from mvn_rocm import synth
    vb = synth.volumetric_batch(2, n_views=n_views, channels=channels, heatmap=64, volume=volume, seed=seed)
    rng = np.random.default_rng(seed)
    cls = channel_classes(channels, cycle)
    off = np.zeros((n_views, channels), np.float32)
    odd = np.arange(n_views) % 2 == 1
    for blk in range((channels + 3) // 4):
        k = int(cls[4 * blk])
        if k == 1:
            o = rng.uniform(88.0, 110.0, n_views) * np.where(odd, 1.0, -1.0)
            o[1] = 100.0
        elif k == 2:
            o = -rng.uniform(75.0, 100.0, n_views)
        elif k == 3:
            o = rng.uniform(-72.0, 84.0, n_views)
        else:
            continue
        off[:, 4 * blk:4 * blk + 4] = o[:, None]
    feat = vb.features.numpy().copy()
    feat[1] += off[:, :, None, None]
    features, base = torch.from_numpy(feat).to(dtype), vb.features.to(dtype)
    coords = vb.coords
    if cuboid:
        from oracle import restate_np
        coords = torch.from_numpy(restate_np.coord_volumes(vb.base_points64, synth.CUBOID_SIDE, volume, vb.thetas,
                                                           "coco", False))
    if crop is not None:
        coords = coords[:, :crop[0], :crop[1], :crop[2]].contiguous()
    proj = vb.proj

    # ---- self-check (CPU): where the denominators fall
    den = 0.0
    for v in range(n_views):
        s = _oracle(features[:, v:v + 1], proj[:, v:v + 1].numpy(), coords.numpy(), "sum")
        den = den + np.exp2(s.astype(np.float64) * LOG2E)
    out = (den > DEN_HI) | (den < DEN_LO)
    share, edge = {}, [np.inf, -np.inf]
    assert not out[0].any(), f"frame 0: {int(out[0].sum())} denominators out of range"
    for blk in range((channels + 3) // 4):
        k, d = int(cls[4 * blk]), den[1, 4 * blk:4 * blk + 4]
        if k in (0, 3):
            assert not out[1, 4 * blk:4 * blk + 4].any(), f"block {blk} (class {k}): denominators out of range"
            edge = [min(edge[0], float(np.log2(d.min()))), max(edge[1], float(np.log2(d.max())))]
        else:
            trip = float((d > DEN_HI).mean() if k == 1 else (d < DEN_LO).mean())
            share[blk] = trip
            assert 0.20 <= trip <= 0.98, f"block {blk} (class {k}): {trip:.3f} of the denominators trip"
    ref = _oracle(features, proj.numpy(), coords.numpy())
    assert np.isfinite(ref).all()
    ref.setflags(write=False)
    return SimpleNamespace(features=features, base=base, proj=proj, coords=coords, classes=cls, ref=ref,
                           trip_share=share, base_points64=vb.base_points64, thetas=vb.thetas, volume=volume,
                           in_range_log2_den=tuple(edge))


# ----------------------------------------------------------------------------- the kernels under test
def _kernel(views, maps, out, layout, channels, tile, lim):
    return SimpleNamespace(views=views, maps=maps, out=out, layout=layout, channels=channels, tile=tile, lim=lim)


F32, BF16 = torch.float32, torch.bfloat16
# tile = the voxel tile of the instantiation the call launches (X4Shape in unproject_x4.hip), lim = the
# slots of one of its LDS buffers that hold pixels (SLOTS - 66)
DEFERRED = {
    "f32_ncdhw": _kernel(4, F32, F32, "ncdhw", 16, (4, 8, 16), 1982),           # <float, float, 0, 0, 1>
    "bf16_ncdhw_bf16": _kernel(4, BF16, BF16, "ncdhw", 16, (8, 8, 8), 1470),    # <u16, u16, 4, 0, 1>
    "bf16_ncdhw_f32": _kernel(4, BF16, F32, "ncdhw", 16, (8, 8, 8), 1470),      # <u16, float, 4, 0, 1>
    "bf16_cl_bf16": _kernel(4, BF16, BF16, "cl", 16, (8, 8, 8), 1982),          # <u16, u16, 2, 1, 1>
    "bf16_cl_f32": _kernel(4, BF16, F32, "cl", 16, (8, 8, 8), 1982),            # <u16, float, 2, 1, 1>
    "bf16_cl_bf16_c12": _kernel(4, BF16, BF16, "cl", 12, (8, 8, 8), 1982),      # the tail-group stores
    "bf16_cl_f32_c12": _kernel(4, BF16, F32, "cl", 12, (8, 8, 8), 1982),
}
PER_GROUP = {
    "f32_cl_f32": _kernel(4, F32, F32, "cl", 16, (4, 8, 16), 1982),             # <float, float, 0, 1, 1>
    "f32_cl_bf16": _kernel(4, F32, BF16, "cl", 16, (4, 8, 16), 1982),           # the same + one device cast
    "f32_8v": _kernel(8, F32, F32, "ncdhw", 16, (4, 8, 8), 1982),               # <float, float, 3, 0, 1>
    "bf16_8v_f32": _kernel(8, BF16, F32, "ncdhw", 16, (4, 8, 8), 1982),         # <u16, float, 3, 0, 1>
    "bf16_8v_bf16": _kernel(8, BF16, BF16, "ncdhw", 16, (4, 8, 8), 1982),       # <u16, u16, 3, 0, 1>
}
# Variants.  'v16': the 16^3 volume on 64^2 maps — every tile's views together exceed one LDS buffer
# (tile_footprints), so its blocks run the multi-pass staging or, where one view alone is too large,
# the global gather.  'ragged': a (13, 21, 10) corner of a 24^3 volume, partial tiles, mostly one
# pass.  'v32': 32^3, default budget: single-pass and multi-pass tiles.  'lds_multipass',
# 'global_fallback': 32^3 with the LDS slot budget chosen as test_fast_every_staging_path does.
VARIANTS = ("ragged", "v32", "lds_multipass", "global_fallback")
SEEDS = {(8, "ragged"): 14}       # seed 12 elsewhere; (8 views, ragged): seed 12 trips every class-1 voxel


def _case(k, variant, kind="explicit"):
    volume, crop = {"v16": (16, None), "ragged": (24, RAGGED)}.get(variant, (32, None))
    return guard_inputs(k.views, k.channels, volume, SEEDS.get((k.views, variant), 12), k.maps, crop,
                        kind == "cuboid")


def _budget(k, g, variant):
    """The LDS slot budget of a variant (0 = the kernel's own) with the precondition asserts of
    test_fast_every_staging_path, and the paths the offset frame's tiles must take."""
    areas = tile_footprints(g.proj.numpy(), g.coords.numpy(), 64, 64, k.tile)
    f1 = areas[len(areas) // 2:]                  # frame 1's tiles
    budget = 0
    if variant == "lds_multipass":
        budget = int(areas.max()) + 64
        assert budget <= k.lim
        assert (areas.sum(1) + 1 > budget).any() and (f1.sum(1) > budget + 64).any()
    elif variant == "global_fallback":
        budget = int(np.median(areas[areas > 0]))
        assert (areas.max(1) > budget - 1).any() and (areas.max(1) <= budget - 1).any()
        assert (f1.max(1) <= budget - 64).any()   # frame 1 keeps staged tiles (the guard runs there)
    elif variant == "v16":
        assert (f1.sum(1) > k.lim + 64).all() and (f1.max(1) <= k.lim - 64).any()
    else:
        assert (f1.sum(1) <= k.lim - 64).any()    # single-pass tiles in the offset frame
    return budget


def _run(k, feat, proj, coords, device):
    """The fast softmax call of kernel ``k``, returned as a (B, C, Vx, Vy, Vz) view."""
    from mvn_rocm import op, v2v
    if k.layout == "cl":
        out = v2v.unproject_channels_last(feat.to(device), proj.to(device), coords, "softmax", out_dtype=k.out,
                                          precision="fast")
        assert out.shape[-1] == feat.shape[2] and out.is_contiguous()
        return out.permute(0, 4, 1, 2, 3)
    return op.unproject_heatmaps(feat.to(device), proj.to(device), coords, "softmax", out_dtype=k.out,
                                 precision="fast")


def _coords(g, kind, device, frames=slice(None)):
    if kind == "explicit":
        return g.coords[frames].to(device)
    from mvn_rocm import synth, volumetric
    # (the oracle ran on restate_np's coordinate volume of these cuboids: guard_inputs(cuboid=True))
    return volumetric.build_cuboids(g.base_points64[frames], synth.CUBOID_SIDE, g.volume, g.thetas[frames],
                                    device=device)


def _bar_ratios(out, ref, maps, classes):
    """error / bar of frame 0 and of each 4-channel block of frame 1 (module docstring)."""
    got = out.float().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    parts = [("frame 0", 0, slice(None))]
    parts += [(f"frame 1, block {b} (class {classes[4 * b]})", 1, slice(4 * b, 4 * b + 4))
              for b in range((ref.shape[1] + 3) // 4)]
    ratios = {}
    for name, f, sl in parts:
        r, e = ref[f, sl].astype(np.float64), np.abs(got[f, sl] - ref[f, sl])
        if maps == F32:
            bound = F32_TOL * np.abs(r).max()
        elif out.dtype == F32:
            bound = bf16_bar("softmax") * np.abs(r).max()
        else:                                     # assert_bf16_fast's bound
            _, ex = np.frexp(r)
            bound = np.where(r == 0, 0.0, np.ldexp(1.0, ex - 8)) + bf16_bar("softmax") * np.abs(r).max()
        ratios[name] = float((e / bound).max())
    return ratios


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int16 if a.dtype == BF16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


def _check_guard(k, variant, kind, device, per_group):
    from mvn_rocm import _lib
    g = _case(k, variant, kind)
    budget = _budget(k, g, variant)
    if k.maps == F32 and k.out == BF16:
        # f32 maps into a bf16 volume: the f32 kernel's volume rounded by one device cast
        # (v2v.unproject_channels_last) — held to the f32 bar before the cast, and the cast exact
        k32 = _kernel(k.views, k.maps, F32, k.layout, k.channels, k.tile, k.lim)
    else:
        k32 = None
    with _lib.unproject_knobs(budget):
        out = _run(k, g.features, g.proj, _coords(g, kind, device), device)
        alone = _run(k, g.features[:1], g.proj[:1], _coords(g, kind, device, slice(0, 1)), device)
        plain = _run(k, g.base, g.proj, _coords(g, kind, device), device) if per_group else None
        out32 = _run(k32, g.features, g.proj, _coords(g, kind, device), device) if k32 else None
    assert out.dtype == k.out and tuple(out.shape) == g.ref.shape
    assert torch.isfinite(out.float()).all()
    if k32:
        assert _bits_equal(out, out32.to(BF16))
        ratios = _bar_ratios(out32, g.ref, k.maps, g.classes)
    else:
        ratios = _bar_ratios(out, g.ref, k.maps, g.classes)
    print(variant, kind, {n: round(r, 3) for n, r in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # frame 0 of the two-frame call = frame 0 unprojected alone: a trip in frame 1 touched nothing of it
    assert _bits_equal(out[:1], alone)
    if per_group:
        # a group's redo leaves the other groups alone: frame 1's class-0 blocks are those of the
        # same call without the offsets, bit for bit
        c0 = torch.from_numpy(g.classes == 0).to(device)
        assert _bits_equal(out[1][c0], plain[1][c0])
        assert _bits_equal(out[0], plain[0])


# ----------------------------------------------------------------------------- the guards
@pytest.mark.parametrize("kind", ("explicit", "cuboid"))
@pytest.mark.parametrize("name", tuple(DEFERRED))
def test_deferred_guard(device, name, kind):
    """4 views, bf16 maps or f32 maps written NCDHW: two frames, the second with out-of-range
    channel blocks beside in-range ones (guard_inputs), 16^3, coordinates read or formed
    in-kernel — the fallback's frame pointers, its cuboid branch, its channels-last stores, and
    voxels of which only some groups are out of range."""
    _check_guard(DEFERRED[name], "v16", kind, device, per_group=False)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ("f32_ncdhw", "bf16_ncdhw_bf16"))
def test_deferred_guard_staging_and_ragged(device, name, variant):
    """The deferred fallback after a single staging pass, after several (its second call site),
    beside the global-gather blocks, and in partial tiles (inactive lanes carry voxel 0)."""
    _check_guard(DEFERRED[name], variant, "explicit", device, per_group=False)


@pytest.mark.parametrize("name", tuple(DEFERRED))
def test_deferred_in_range_extremes_without_help(device, name):
    """A tripping voxel of a deferred kernel takes its wave along, so beside class-1 and class-2
    blocks the class-3 blocks are rewritten by the exact path too.  Here the offset frame holds
    only classes 0 and 3 (nothing trips, guard_inputs checks it): offsets up to +84 and down to -72
    go through the max-free form alone and meet the same bars (32^3: staged blocks throughout)."""
    k = DEFERRED[name]
    g = guard_inputs(k.views, k.channels, 32, 12, k.maps, cycle=(0, 3, 3, 3))
    assert not g.trip_share and g.in_range_log2_den[1] > 100.0
    out = _run(k, g.features, g.proj, g.coords.to(device), device)
    assert torch.isfinite(out.float()).all()
    ratios = _bar_ratios(out, g.ref, k.maps, g.classes)
    print("log2 den in", g.in_range_log2_den, {n: round(r, 3) for n, r in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", tuple(PER_GROUP))
def test_per_group_guard(device, name):
    """8 views, and 4 views of f32 maps written channels-last: a group out of range redoes itself
    max-first and leaves the other groups' values as they were."""
    _check_guard(PER_GROUP[name], "v16", "explicit", device, per_group=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ("f32_cl_f32", "f32_8v"))
def test_per_group_guard_staging_and_ragged(device, name, variant):
    _check_guard(PER_GROUP[name], variant, "explicit", device, per_group=True)


# ----------------------------------------------------------------------------- kernels never launched: parity
@functools.lru_cache(maxsize=None)
def _unit_inputs(volume, dtype, channels=8, ragged=False):
    from mvn_rocm import synth
    vb = synth.volumetric_batch(1, channels=channels, heatmap=64, volume=volume, seed=61, dtype=dtype)
    coords = vb.coords[:, :RAGGED[0], :RAGGED[1], :RAGGED[2]].contiguous() if ragged else vb.coords
    conf = np.random.default_rng(61).uniform(0.05, 1.0, (1, 4, channels)).astype(np.float32)
    return vb.features, vb.proj, coords, conf


@functools.lru_cache(maxsize=None)
def _unit_ref(volume, dtype, channels, ragged, method, ac):
    feat, proj, coords, conf = _unit_inputs(volume, dtype, channels, ragged)
    ref = _oracle(feat, proj.numpy(), coords.numpy(), method, conf=conf, align_corners=int(ac))
    ref.setflags(write=False)
    return ref


def _both_layouts(device, feat, proj, coords, conf, method, ac, out_dtype):
    """(channels-last fast volume as NCDHW view, fast NCDHW volume) of one call."""
    from mvn_rocm import op, v2v
    f, P, c, cf = feat.to(device), proj.to(device), coords.to(device), torch.from_numpy(conf).to(device)
    cl = v2v.unproject_channels_last(f, P, c, method, out_dtype=out_dtype, align_corners=ac, vol_confidences=cf,
                                     precision="fast")
    nc = op.unproject_heatmaps(f, P, c, method, cf, align_corners=ac, out_dtype=out_dtype, precision="fast")
    assert cl.is_contiguous() and tuple(cl.shape) == tuple(nc.permute(0, 2, 3, 4, 1).shape)
    return cl.permute(0, 4, 1, 2, 3), nc


def _check_f32_channels_last(device, method, ac, volume, ragged):
    feat, proj, coords, conf = _unit_inputs(volume, F32, 8, ragged)
    ref = _unit_ref(volume, F32, 8, ragged, method, ac)
    cl, nc = _both_layouts(device, feat, proj, coords, conf, method, ac, F32)
    assert max_rel(cl.cpu().numpy(), ref) <= F32_TOL
    # the same tile and arithmetic in both layouts (the two softmax guards differ only where they trip)
    assert _bits_equal(cl, nc)
    assert 0.2 < (ref != 0).mean()


@pytest.mark.parametrize("volume", (16, 32))
@pytest.mark.parametrize("ac", (False, True))
@pytest.mark.parametrize("method", METHODS)
def test_fast_f32_channels_last_parity(device, method, ac, volume):
    """unproject_x4<AGG, float, float, 0, CL, FAST> (v2v.unproject_channels_last on f32 maps): one
    frame of 4 views x 8 ch x 64^2 into 16^3 (multi-pass and gather blocks) and 32^3 (single-pass
    blocks too), every aggregation, both align_corners: the f32 bar against the oracle, and the
    fast NCDHW volume transposed bit for bit."""
    _check_f32_channels_last(device, method, ac, volume, False)


@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_fast_f32_channels_last_ragged(device, method):
    """The same on a (13, 21, 10) volume: partial tiles on every axis."""
    _check_f32_channels_last(device, method, False, 24, True)


@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_fast_bf16_maps_f32_channels_last_parity(device, method):
    """unproject_x4<AGG, uint16_t, float, 2, CL, FAST>: bf16 maps into an f32 channels-last volume —
    the bf16 bar against the oracle on the same bits, and the fast NCDHW out_dtype=float32 volume
    transposed bit for bit (32^3: every footprint fits both kernels' LDS buffers, so both stage
    every block)."""
    feat, proj, coords, conf = _unit_inputs(32, BF16, 8)
    ref = _unit_ref(32, BF16, 8, False, method, False)
    cl, nc = _both_layouts(device, feat, proj, coords, conf, method, False, F32)
    assert cl.dtype == F32
    assert max_rel(cl.cpu().numpy(), ref) <= bf16_bar(method)
    assert _bits_equal(cl, nc)
    assert 0.2 < (ref != 0).mean()


@pytest.mark.parametrize("channels", (12, 20))
def test_fast_bf16_channels_last_tail_group(device, channels):
    """bf16 channels-last, fast, C / 4 not a multiple of 4: the voxel record's tail goes out as
    8-byte stores (the `c0 + G >= C` branch of store_out) — the fast NCDHW volume transposed bit for
    bit, within the bf16 bar of the oracle."""
    feat, proj, coords, conf = _unit_inputs(32, BF16, channels)
    ref = _unit_ref(32, BF16, channels, False, "softmax", False)
    cl, nc = _both_layouts(device, feat, proj, coords, conf, "softmax", False, BF16)
    assert cl.dtype == BF16
    assert _bits_equal(cl, nc)
    assert_bf16_fast(cl, ref, "softmax")


# ----------------------------------------------------------------------------- +-inf maps
@pytest.mark.parametrize("n_views", (4, 8))
def test_fast_inf_features_as_the_reference(device, n_views):
    """+inf and -inf pixels (f32 maps; 4 views: the deferred guard, 8 views: the per-group guard):
    the non-finite voxels are the oracle's, except where the fast projection's floor lands on the
    other side of a pixel edge (the allowance of test_fast_nan_features_propagate), and the finite
    remainder meets the f32 bar.  (+inf overflows the max-free denominator and trips the guard; the
    max-first form then gives the reference's NaN.)"""
    from mvn_rocm import op, synth
    vb = synth.volumetric_batch(1, n_views=n_views, channels=8, volume=32, seed=13)
    feat = vb.features.clone()
    feat[0, 1, 2, 40:44, 50:53] = float("inf")
    feat[0, 3, :, 10, 10] = float("-inf")
    ref = capi.unproject(feat.numpy(), vb.proj.numpy(), vb.coords.numpy(), "softmax")
    got = op.unproject_heatmaps(feat.to(device), vb.proj.to(device), vb.coords.to(device), "softmax",
                                precision="fast").cpu().numpy()
    nr, ng = ~np.isfinite(ref), ~np.isfinite(got)
    assert nr.sum() > 50
    assert (nr != ng).sum() <= max(4, nr.sum() // 50)
    assert (np.isnan(ref) != np.isnan(got)).sum() <= max(4, nr.sum() // 50)
    fin = ~(nr | ng)
    assert max_rel(got[fin], ref[fin]) <= F32_TOL
