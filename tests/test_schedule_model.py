"""tools/schedule_model.py (CPU): its per-tile chunk counts against tools/footprints.py, the
multi-pass tiles of the bench launch at the former and the present LDS slot limit, and the
replay's bookkeeping."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import footprints  # noqa: E402
import lds_conflicts  # noqa: E402
import schedule_model  # noqa: E402


@pytest.fixture(scope="module")
def bench_geometry():
    return lds_conflicts.geometry(B=8)


def test_chunk_counts_of_frame_0_equal_footprints(bench_geometry):
    fx, fy, ok = (a[:1] for a in bench_geometry)
    lim = schedule_model.image_slots()
    chunks, slots, passes = schedule_model.tiles(fx, fy, ok, lim)
    s, c, slow = footprints.tile_stats(fx, fy, ok, schedule_model.TILE, 512, lim + 66)
    assert np.array_equal(chunks, c)
    assert np.array_equal(slots, s)
    assert int((passes != 1).sum()) == slow


def test_no_bench_tile_is_multi_pass_at_the_present_limit(bench_geometry):
    lim = schedule_model.image_slots()
    chunks, slots, passes = schedule_model.tiles(*bench_geometry, lim)
    assert chunks.size == 8 * 512
    assert (passes == 1).all()
    assert slots.max() <= lim and chunks.max() <= schedule_model.KCAP
    # at the former 2,048-slot buffers: 43 tiles, in two frames
    old = schedule_model.tiles(*bench_geometry, 2048 - 66)[2].reshape(8, 512)
    assert (old != 1).sum(1).tolist() == [0, 11, 0, 0, 32, 0, 0, 0]


def test_replay_accounts_for_every_block():
    """Equal costs: 512 tiles per frame fill the 8 x 64 slots exactly, efficiency 1; one costly
    tile stretches the makespan by its excess, whatever the order."""
    order = schedule_model.block_tiles(-1, 2, (16, 8, 4))
    cost = np.ones(order.size)
    assert schedule_model.simulate(order, cost) == (2.0, 1.0)
    cost[order[-1]] = 3.0
    mk, eff = schedule_model.simulate(order, cost)
    assert mk == 4.0 and eff == pytest.approx((order.size + 2) / (512 * 4.0))
    assert schedule_model.simulate(order, cost, pooled=True)[0] == 4.0
