"""The four-view f32 unprojection on 8-byte LDS slots of 2 channels (X4Shape<5> in
csrc/unproject_x4.hip: shape 0's tile, footprints and pass limit at 3 blocks per CU), the kernel
of every 4-view f32 NCDHW call in exact arithmetic.

References.  Bits: the generic tiled kernel (unproject_knobs(generic=True)) and the 16-byte-slot
kernel, shape 0 (unproject_knobs(wide_slots=True)); the three agree bit for bit for every
aggregation.  Values: the C oracle, 'sum' / 'max' / 'conf' exact, softmax <= 1e-5 of max|ref|.

The channel loop handles two 2-channel groups per trip, so C = 4, 8, 12 are one, two and three
trips, with the exit after the first group of a trip never taken (C % 4 == 0) and the exit after
the second taken at the first or a later trip.  The staging cases are asserted on the CPU by
restating the kernel's footprint rule (test_gpu_x4_prologue._tiles) at limits moved by a margin,
as tests/test_gpu_x4_lds.py does.  MI355X only."""
import ctypes
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import test_gpu_x4_prologue as prologue
from conftest import assert_bits_equal, assert_parity_with_nans, max_rel
from oracle import capi, restate_np
from test_gpu_x4_prologue import METHODS, SHAPES, _coords

THREADS, KCAP = SHAPES["f32"]["threads"], SHAPES["f32"]["kcap"]
MARGIN = 128                       # slots: the kernel forms the boxes in f32, the model in f64
PAYLOAD = 0x7FC12345               # a quiet NaN no kernel produces
ERR_ARG = -1                       # MVN_ERR_ARG (include/mvn_hip.h)


def _lib():
    from mvn_rocm import _lib
    return _lib


def _launch(F, P, X, cf, method, vol, ac=False, channels_last=False, out=None, **knobs):
    """mvn_unproject_ex through the C ABI into `out` (default: a NaN-filled f32 buffer)."""
    L = _lib()
    lib = L.load()
    B, N, C, H, W = F.shape
    Vx, Vy, Vz = vol
    if out is None:
        out = torch.full((B, Vx, Vy, Vz, C) if channels_last else (B, C, Vx, Vy, Vz), float("nan"),
                         dtype=torch.float32, device=F.device)
    code = L.MVN_DTYPE_BF16 if F.dtype == torch.bfloat16 else L.MVN_DTYPE_F32
    with L.unproject_knobs(**knobs):
        L.check(lib.mvn_unproject_ex(
            F.data_ptr(), code, P.data_ptr(), X.data_ptr(), cf.data_ptr(), out.data_ptr(), L.MVN_DTYPE_F32,
            L.MVN_LAYOUT_NDHWC if channels_last else L.MVN_LAYOUT_NCDHW, B, N, C, H, W, Vx, Vy, Vz,
            METHODS.index(method), int(ac), torch.cuda.current_stream().cuda_stream), "mvn_unproject_ex")
        torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _three(F, P, X, cf, method, vol, ac=False, **knobs):
    """The 2-channel-slot kernel's output, equal in bits to the generic kernel's and to shape 0's."""
    a = _launch(F, P, X, cf, method, vol, ac, **knobs)
    g = _launch(F, P, X, cf, method, vol, ac, generic=True, **knobs)
    w = _launch(F, P, X, cf, method, vol, ac, wide_slots=True, **knobs)
    assert torch.equal(_bits(a), _bits(g)), f"{method}: differs from the generic kernel"
    assert torch.equal(_bits(a), _bits(w)), f"{method}: differs from the 16-byte-slot kernel"
    return a


def _against_oracle(got, ref, method):
    if np.isnan(ref).any():
        assert_parity_with_nans(got, ref, method)
    elif method == "softmax":
        assert max_rel(got, ref) <= 1e-5
    else:
        assert_bits_equal(got, ref)


def _to(device, *arrays):
    return tuple(torch.tensor(a, device=device) for a in arrays)


# ---- resources -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_blocks_per_cu_without_scratch(device):
    lib = _lib().load()
    priv, regs = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.mvn_debug_x4_shape_occupancy(5, ctypes.byref(priv), ctypes.byref(regs)) == 3
    assert priv.value == 0 and 0 < regs.value <= 80, (priv.value, regs.value)
    assert lib.mvn_debug_x4_shape_occupancy(0, ctypes.byref(priv), ctypes.byref(regs)) == 2
    assert lib.mvn_debug_unproject_occupancy(0) == 2


def test_shape_occupancy_arguments():
    lib = _lib().load()
    v = ctypes.c_int(0)
    for shape in (-1, 1, 2, 3, 4, 6):
        assert lib.mvn_debug_x4_shape_occupancy(shape, ctypes.byref(v), ctypes.byref(v)) == ERR_ARG
    assert lib.mvn_debug_x4_shape_occupancy(5, None, ctypes.byref(v)) == ERR_ARG
    assert lib.mvn_debug_x4_shape_occupancy(5, ctypes.byref(v), None) == ERR_ARG


# ---- loop exits and ragged tiles on small maps --------------------------------------------------
def _small_proj(rng, frames, H, W):
    """Ring cameras at a 16-pixel heatmap, rows scaled to an H x W map (the volume below spans it
    and some voxels fall outside)."""
    from mvn_rocm import synth
    proj = synth.projections(synth.ring_cameras(4, rng), heatmap_size=16).copy()
    proj[:, 0] *= W / 16.0
    proj[:, 1] *= H / 16.0
    return np.repeat(proj[None], frames, 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _small_case(hw, channels, vol):
    H, W = hw
    rng = np.random.default_rng(1000 * H + 10 * channels + vol[0])
    proj = _small_proj(rng, 2, H, W)
    Vx, Vy, Vz = vol
    g = np.stack(np.meshgrid(np.arange(Vx) - (Vx - 1) / 2.0, np.arange(Vy) - (Vy - 1) / 2.0,
                             np.arange(Vz) - (Vz - 1) / 2.0, indexing="ij"), -1)
    coords = np.stack([np.array([0.0, 0.0, 900.0]) + s * g for s in (150.0, 210.0)]).astype(np.float32)
    feat = rng.standard_normal((2, 4, channels, H, W)).astype(np.float32)
    conf = rng.uniform(0.05, 1.0, (2, 4, channels)).astype(np.float32)
    refs = {(m, ac): capi.unproject(feat, proj, coords, m, conf, ac) for m in METHODS for ac in (False, True)}
    for a in (proj, coords, feat, conf) + tuple(refs.values()):
        a.setflags(write=False)
    return proj, coords, feat, conf, refs


@pytest.mark.gpu
@pytest.mark.parametrize("vol", ((4, 8, 16), (5, 9, 17)), ids=lambda v: "v{}x{}x{}".format(*v))
@pytest.mark.parametrize("channels", (4, 8, 12))
@pytest.mark.parametrize("hw", ((12, 16), (16, 12)), ids=lambda s: "h{}w{}".format(*s))
def test_loop_exits_and_ragged_tiles(device, hw, channels, vol):
    proj, coords, feat, conf, refs = _small_case(hw, channels, vol)
    assert any((r != 0).any() for r in refs.values()) and (refs[("sum", False)] == 0).any()
    F, P, X, cf = _to(device, feat, proj, coords, conf)
    for ac in (False, True):
        for m in METHODS:
            a = _three(F, P, X, cf, m, vol, ac)
            assert not torch.isnan(a).any(), "a voxel was not written"
            _against_oracle(a.cpu().numpy(), refs[(m, ac)], m)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_in_kernel_cuboid_coordinates(device, method):
    """Coordinates formed in-kernel from per-frame cuboids (V = 12: partial tiles in y and z)."""
    from mvn_rocm import op, volumetric
    L = _lib()
    rng = np.random.default_rng(5)
    H, W, C, V = 16, 12, 12, 12
    proj = _small_proj(rng, 2, H, W)
    base, theta = rng.uniform(-200, 200, (2, 3)) + np.array([0, 0, 900.0]), rng.uniform(0, 2 * np.pi, 2)
    feat = rng.standard_normal((2, 4, C, H, W)).astype(np.float32)
    conf = rng.uniform(0.05, 1.0, (2, 4, C)).astype(np.float32)
    ref = capi.unproject(feat, proj, restate_np.coord_volumes(base, 2500.0, V, theta, "coco", False), method, conf)
    cub = volumetric.build_cuboids(base, 2500.0, V, theta, device=device)
    F, P, cf = _to(device, feat, proj, conf)
    outs = []
    for knobs in ({}, dict(generic=True), dict(wide_slots=True)):
        with L.unproject_knobs(**knobs):
            outs.append(op.unproject_heatmaps(F, P, cub, method, cf))
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
    _against_oracle(outs[0].cpu().numpy(), ref, method)


# ---- the three staging paths and the second chunk slot -----------------------------------------
# lattice classes of _coords (voxel spacing in mm): small footprints; narrow tall ones (more
# chunks than threads within one buffer); several passes; a single view above the buffer
SPACING = ((18, 18, 18), (10, 10, 125), (80, 80, 80), (120, 120, 120))
VOL, FRAMES, HEATMAP, CHANNELS = (8, 16, 32), 2, 96, 8


def _passes(proj, coords, lim):
    with mock.patch.object(prologue, "LIM", lim):
        return prologue._tiles(proj, coords, HEATMAP, HEATMAP, SHAPES["f32"]["tile"], THREADS, KCAP)


@functools.lru_cache(maxsize=None)
def _staging_case():
    from mvn_rocm import synth
    rng = np.random.default_rng(78)
    proj = np.repeat(synth.projections(synth.ring_cameras(4, rng), heatmap_size=HEATMAP)[None], FRAMES, 0)
    proj = proj.astype(np.float32)
    coords = _coords(FRAMES, VOL, SPACING, HEATMAP)
    feat = rng.standard_normal((FRAMES, 4, CHANNELS, HEATMAP, HEATMAP)).astype(np.float32)
    conf = rng.uniform(0.05, 1.0, (FRAMES, 4, CHANNELS)).astype(np.float32)
    refs = {m: capi.unproject(feat, proj, coords, m, conf) for m in METHODS}
    for a in (proj, coords, feat, conf) + tuple(refs.values()):
        a.setflags(write=False)
    return proj, coords, feat, conf, refs


def test_tiles_cover_the_staging_paths_and_both_chunk_slots():
    """(chunk total of the first pass, passes or -1, a view without a sample) per tile, at the pass
    limit of the kernel (2,366 image slots, shape 0's) moved down and up by the margin."""
    proj, coords = _staging_case()[:2]
    lim = _lib().load().mvn_debug_x4_image_slots(0)
    assert lim == 2432 - 66
    lo, hi = _passes(proj, coords, lim - MARGIN), _passes(proj, coords, lim + MARGIN)
    both = list(zip(lo, hi))
    assert any(a[1] == b[1] == 1 and 0 < b[0] <= THREADS - 32 for a, b in both), "no one-pass tile within the first chunk slot"
    assert any(a[1] == b[1] == 1 and THREADS + 32 <= a[0] and b[0] <= KCAP - 32 for a, b in both), \
        "no one-pass tile with both chunk slots live"
    assert any(a[1] > 1 and b[1] > 1 for a, b in both), "no tile that takes several passes"
    assert any(a[1] == b[1] == -1 for a, b in both), "no tile on the gather fallback"


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_staging_paths(device, method):
    proj, coords, feat, conf, refs = _staging_case()
    F, P, X, cf = _to(device, feat, proj, coords, conf)
    a = _three(F, P, X, cf, method, VOL)
    assert not torch.isnan(a).any(), "a voxel was not written"
    _against_oracle(a.cpu().numpy(), refs[method], method)


@pytest.mark.gpu
@pytest.mark.parametrize("budget", ("multipass", "fallback"))
@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_staging_paths_under_the_lds_knob(device, method, budget):
    """The small-map case with the slot budget lowered: below the views' sum (several passes), and
    below the largest single view (global gather)."""
    from test_gpu_parity import tile_footprints
    vol, hw = (5, 9, 17), (16, 12)
    proj, coords, feat, conf, refs = _small_case(hw, 12, vol)
    areas = tile_footprints(proj, coords, hw[0], hw[1], (4, 8, 16))
    if budget == "multipass":
        slots = int(areas.max()) + 64
        assert (areas.sum(1) + 1 > slots).any()
    else:
        slots = int(np.median(areas[areas > 0]))
        assert (areas.max(1) > slots - 1).any() and (areas.max(1) <= slots - 1).any()
    F, P, X, cf = _to(device, feat, proj, coords, conf)
    a = _three(F, P, X, cf, method, vol, lds_slots=slots)
    _against_oracle(a.cpu().numpy(), refs[(method, False)], method)


# ---- edges of the function -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_voxels_that_sample_nothing_are_plus_zero(device, method):
    """x-planes 0-1 far above the ring (behind every camera), 2-4 far below (in front, outside
    every image): every output is +0, bits and all."""
    proj, _, feat, conf, _ = _small_case((12, 16), 8, (5, 9, 17))
    coords = np.zeros((2, 5, 9, 17, 3), np.float32)
    coords[..., :2] = np.random.default_rng(3).uniform(-300, 300, coords.shape[:-1] + (2,))
    coords[:, :2, ..., 2] = 1e6
    coords[:, 2:, ..., 2] = -1e5
    ref = capi.unproject(feat, proj, coords, method, conf)
    assert not ref.view(np.uint32).any()
    F, P, X, cf = _to(device, feat, proj, coords, conf)
    a = _three(F, P, X, cf, method, (5, 9, 17))
    assert not _bits(a).any()


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_nan_pixels_and_a_view_outside(device, method):
    """NaN pixels give the generic kernel's bits (and NaN where the oracle has it); view 3's
    principal point moved 10,000 pixels away, so no voxel samples it."""
    vol = (5, 9, 17)
    proj, coords, feat, conf, _ = _small_case((16, 12), 12, vol)
    proj, feat = proj.copy(), feat.copy()
    proj[:, 3, 0] += 1e4 * proj[:, 3, 2]
    tiles = prologue._tiles(proj, coords, 16, 12, (4, 8, 16), THREADS, KCAP)
    assert all(t[2] for t in tiles) and any(t[0] > 0 for t in tiles)
    feat.reshape(-1)[np.random.default_rng(9).choice(feat.size, 40, replace=False)] = np.nan
    ref = capi.unproject(feat, proj, coords, method, conf)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    F, P, X, cf = _to(device, feat, proj, coords, conf)
    a = _three(F, P, X, cf, method, vol)
    _against_oracle(a.cpu().numpy(), ref, method)


# ---- memory discipline -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method", ("sum", "softmax"))
def test_output_between_guards(device, method):
    vol, C = (5, 9, 17), 12
    proj, coords, feat, conf, refs = _small_case((16, 12), C, vol)
    n, guard = 2 * C * 5 * 9 * 17, 1024
    buf = torch.full((guard + n + guard,), PAYLOAD, dtype=torch.int32, device=device)
    out = buf[guard:guard + n].view(torch.float32).view(2, C, *vol)
    assert out.data_ptr() == buf.data_ptr() + 4 * guard
    F, P, X, cf = _to(device, feat, proj, coords, conf)
    _launch(F, P, X, cf, method, vol, out=out)
    assert bool((buf[:guard] == PAYLOAD).all()) and bool((buf[guard + n:] == PAYLOAD).all()), "a guard was written"
    assert not bool((buf[guard:guard + n] == PAYLOAD).any()), "an output element was not written"
    _against_oracle(out.cpu().numpy(), refs[(method, False)], method)


# ---- dispatch ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("call", ("f32-ncdhw", "f32-cl", "bf16", "8-views"))
def test_dispatch_under_the_wide_slot_knob(device, call):
    """The knob only chooses between two kernels that agree in bits, so no output tells them
    apart: what is asserted is that every kind of call gives equal outputs with and without it
    and equal to the generic kernel (4-view f32 NCDHW is the one call it re-routes; the resources
    test above shows that the re-routed kernel is the 3-block one)."""
    from mvn_rocm import synth
    n_views = 8 if call == "8-views" else 4
    vb = synth.volumetric_batch(2, n_views=n_views, channels=8, heatmap=32, volume=16, seed=11)
    F = vb.features.to(device)
    if call == "bf16":
        F = F.to(torch.bfloat16)
    P, X = vb.proj.to(device), vb.coords.to(device)
    cf = torch.ones((2, n_views, 8), device=device)
    kw = dict(channels_last=call == "f32-cl")
    a = _launch(F, P, X, cf, "softmax", (16, 16, 16), **kw)
    w = _launch(F, P, X, cf, "softmax", (16, 16, 16), wide_slots=True, **kw)
    g = _launch(F, P, X, cf, "softmax", (16, 16, 16), generic=True, **kw)
    assert not torch.isnan(a).any()
    assert torch.equal(_bits(a), _bits(w)) and torch.equal(_bits(a), _bits(g))
