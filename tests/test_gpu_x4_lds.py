"""The LDS buffers of the f32 four-view unprojection (X4Shape<0> in csrc/unproject_x4.hip: 2,432
slots, 2,366 of them image slots, two blocks of 78,336 bytes per CU).  Geometry as in
test_gpu_x4_prologue.py (its _coords and _tiles, the latter at the slot limit under test): four
lattices whose tiles' footprints are small; between the former limit of 1,982 image slots and the
new one (one pass now); above the new limit (several passes of whole views); a single view above
it (global-gather fallback).  The three cases are asserted on the CPU with a margin of 128 slots
(that file's 32 chunks of 4 pixels: the kernel forms the boxes in f32, the model in f64) by
evaluating the pass rule at limits moved by the margin.  Every aggregation is compared bitwise
with the generic tiled kernel and with the C oracle within the bars of test_gpu_x4.py."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import test_gpu_x4_prologue as prologue
from conftest import assert_bits_equal, max_rel
from oracle import capi
from test_gpu_x4_prologue import METHODS, SHAPES, _coords, _launch

OLD_LIMIT = 2048 - 66
MARGIN = 128
# voxel spacing (mm) of the four lattice classes of _coords: small, one pass only at the new
# limit, several passes, gather fallback
SPACING = ((18, 18, 18), (56, 56, 56), (80, 80, 80), (120, 120, 120))
VOL, FRAMES, HEATMAP, CHANNELS = (8, 16, 32), 2, 96, 8


def _limit():
    from mvn_rocm import _lib
    return _lib.load().mvn_debug_x4_image_slots(0)


def _passes(proj, coords, lim):
    s = SHAPES["f32"]
    with mock.patch.object(prologue, "LIM", lim):
        return prologue._tiles(proj, coords, HEATMAP, HEATMAP, s["tile"], s["threads"], s["kcap"])


@functools.lru_cache(maxsize=None)
def _case():
    from mvn_rocm import synth
    rng = np.random.default_rng(77)
    cams = synth.ring_cameras(4, rng)
    proj = np.repeat(synth.projections(cams, heatmap_size=HEATMAP)[None], FRAMES, 0).astype(np.float32)
    coords = _coords(FRAMES, VOL, SPACING, HEATMAP)
    feat = rng.standard_normal((FRAMES, 4, CHANNELS, HEATMAP, HEATMAP)).astype(np.float32)
    conf = rng.uniform(0.05, 1.0, (FRAMES, 4, CHANNELS)).astype(np.float32)
    refs = {m: capi.unproject(feat, proj, coords, m, conf) for m in METHODS}
    for a in (proj, coords, feat, conf) + tuple(refs.values()):
        a.setflags(write=False)
    return proj, coords, feat, conf, refs


def test_image_slot_counts_of_the_shapes():
    from mvn_rocm import _lib
    lib = _lib.load()
    assert lib.mvn_debug_x4_image_slots(0) == 2432 - 66
    assert lib.mvn_debug_x4_image_slots(1) == lib.mvn_debug_x4_image_slots(2) == OLD_LIMIT
    assert lib.mvn_debug_x4_image_slots(3) == lib.mvn_debug_x4_image_slots(-1) == -1


def test_tiles_cover_the_three_staging_paths():
    proj, coords = _case()[:2]
    new = _limit()
    assert new - MARGIN > OLD_LIMIT + MARGIN
    kcap = SHAPES["f32"]["kcap"]
    was, lo, hi = (_passes(proj, coords, lim) for lim in (OLD_LIMIT + MARGIN, new - MARGIN, new + MARGIN))
    # (chunk total of the first pass, passes or -1, a view without a sample) per tile
    assert any(w[1] > 1 and a[1] == 1 and 0 < a[0] <= kcap - 32 for w, a in zip(was, lo)), \
        "no tile between the former limit and the new one that takes one pass now"
    assert any(a[1] > 1 and b[1] > 1 for a, b in zip(lo, hi)), "no tile that still takes several passes"
    assert any(b[1] == -1 for b in hi), "no tile on the gather fallback"
    assert any(a[1] == 1 and w[1] == 1 for w, a in zip(was, lo)), "no tile that took one pass before"


@pytest.mark.gpu
def test_two_blocks_per_cu(device):
    """The larger buffers still leave two resident blocks per CU (2 x 78,336 bytes of 160 KB)."""
    from mvn_rocm import _lib
    assert _lib.load().mvn_debug_unproject_occupancy(0) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_staging_paths_equal_generic_kernel_and_oracle(device, method):
    proj, coords, feat, conf, refs = _case()
    F, P, X, cf = (torch.tensor(a, device=device) for a in (feat, proj, coords, conf))
    a = _launch(F, P, X, cf, method, VOL)
    b = _launch(F, P, X, cf, method, VOL, generic=True)
    assert not torch.isnan(a).any(), "a voxel was not written"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = a.cpu().numpy()
    if method == "softmax":
        assert max_rel(got, refs[method]) <= 1e-5
    else:
        assert_bits_equal(got, refs[method])
