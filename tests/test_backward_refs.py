"""The references behind tests/test_gpu_backward_shapes.py, checked on the CPU.

The GPU file's bars are only as good as its references: here the f32-design DLT reference is
pinned against plain float64 autograd (exactly, where the design matrix is exact in f32, and
within the measured sensitivity on the GPU file's own inputs), the f32 reference chains of the
soft-argmax and of the whole training step are shown to sit well inside the GPU bars on exactly
the GPU file's inputs (so a later change of those inputs cannot silently eat the headroom),
and each unprojection geometry is shown to land on the kernel path it is meant for."""
import numpy as np
import pytest
import torch

from oracle import backward_cases as cases
from oracle import restate_torch
from oracle.backward_cases import max_rel_per
from test_gpu_parity import tile_footprints


def test_max_rel_per_normalises_each_slice():
    ref = np.zeros((2, 3, 4))
    ref[0] = 1e6
    ref[1, 0] = 1.0
    out = ref.copy()
    out[1, 0, 2] = 1.5                      # 50% of its own slice, 5e-7 of the global maximum
    assert np.abs(out - ref).max() / np.abs(ref).max() < 1e-6
    got = max_rel_per(out, ref, 2)
    assert got.shape == (2, 3) and got[1, 0] == 0.5 and got[0].max() == 0.0
    assert max_rel_per(out, ref, 1)[1] == 0.5
    out[1, 1, 0] = 0.25                     # a slice whose reference is all zero: absolute
    assert max_rel_per(out, ref, 2)[1, 1] == 0.25


@pytest.mark.parametrize("n_views", (2, 3, 5))
@pytest.mark.parametrize("use_conf", (True, False))
def test_f32_design_reference_is_float64_autograd_on_exact_inputs(n_views, use_conf):
    """Small-integer projections, points and confidences: every product and difference of
    multiview.py:150-152 is exact in f32, so forming A in f32 or in f64 is the same matrix and
    the closed-form chain rule must reproduce autograd's gradients (1e-9 per joint)."""
    rng = np.random.default_rng(n_views)
    B, J = 2, 3
    X = rng.integers(-3, 4, (B, J, 3)).astype(np.float64)
    P = np.zeros((B, n_views, 3, 4))
    for b in range(B):
        for v in range(n_views):
            while True:                     # integer cameras in front of every point
                M = rng.integers(-4, 5, (3, 4)).astype(np.float64)
                M[2, 3] = 40.0
                if np.linalg.matrix_rank(M[:, :3]) == 3:
                    break
            P[b, v] = M
    Xh = np.concatenate([X, np.ones((B, J, 1))], -1)
    uvw = np.einsum("bvrk,bjk->bvjr", P, Xh)
    pts = np.round(uvw[..., :2] / uvw[..., 2:]) + rng.integers(-2, 3, (B, n_views, J, 2))
    conf = rng.integers(1, 5, (B, n_views, J)).astype(np.float64)
    P, pts, conf = torch.from_numpy(P), torch.from_numpy(pts), torch.from_numpy(conf)
    gout = torch.randn((B, J, 3), generator=torch.Generator().manual_seed(1))    # f32: exact in both
    c = conf if use_conf else None
    out, gp, gc = restate_torch.triangulate_batch_of_points_f32_design(P, pts, c, gout)
    p64 = pts.clone().requires_grad_(True)
    c64 = (conf.clone() if use_conf else torch.ones_like(conf)).requires_grad_(True)
    ref = restate_torch.triangulate_batch_of_points(P, p64, c64)
    ref.backward(gout)
    assert np.abs(out.numpy() - ref.detach().numpy()).max() <= 1e-5 * np.abs(out.numpy()).max()   # ref is f32 storage
    assert np.abs(p64.grad.numpy()).max() > 0 and np.abs(c64.grad.numpy()).max() > 0
    # per joint: (B, N, J, ..) -> joints first
    assert max_rel_per(gp.permute(0, 2, 1, 3).numpy(), p64.grad.permute(0, 2, 1, 3).numpy(), 2).max() <= 1e-9
    assert max_rel_per(gc.permute(0, 2, 1).numpy(), c64.grad.permute(0, 2, 1).numpy(), 2).max() <= 1e-9


@pytest.mark.parametrize("n_views", (2, 3, 4, 8))
def test_f32_design_reference_sensitivity_on_the_gpu_inputs(n_views):
    """On the GPU test's inputs the f32 rounding of A moves grad_pts by <= 1e-5 per joint and
    grad_conf by <= 1e-5 per frame for 3-8 views (2 views: the 4 x 4 system's smallest
    singular value is the pixel noise alone; its confidence gradient is only reported)."""
    c = cases.dlt_case(n_views)
    _, gp, gc = restate_torch.triangulate_batch_of_points_f32_design(c["proj"], c["points"], c["conf"], c["gout"])
    rp, rc = cases.dlt_ref_f64(c["proj"], c["points"], c["conf"], c["gout"])
    per_joint = max_rel_per(gp.permute(0, 2, 1, 3).numpy(), np.transpose(rp, (0, 2, 1, 3)), 2).max()
    per_frame = max_rel_per(gc.numpy(), rc, 1).max()
    print(f"n_views={n_views}: grad_pts per joint {per_joint:.2e}, grad_conf per frame {per_frame:.2e}")
    assert per_joint <= 1e-5
    if n_views >= 3:
        assert per_frame <= 1e-5
    if n_views >= 4:
        zero = (c["conf"] == 0).numpy()
        assert zero.any() and (gp.numpy()[zero] == 0).all() and np.isfinite(gc.numpy()[zero]).all()


@pytest.mark.parametrize("softmax,mult", ((True, 1.0), (True, 1.7), (False, 1.7)))
def test_f32_softargmax_reference_headroom(softmax, mult):
    """The f32 reference of the soft-argmax backward stays within 3e-5 per joint of float64
    on the GPU test's inputs (its bar is 1e-4 per joint)."""
    c = cases.softargmax_case()
    args = (c["logits"], c["coords"], softmax, mult, c["grad_xyz"], c["idx"], "full")
    r64 = cases.softargmax_ref_grad(*args)
    r32 = cases.softargmax_ref_grad(*args, dtype=torch.float32)
    worst = max_rel_per(r32, r64, 2).max()
    print(f"softmax={softmax} mult={mult}: f32 vs f64 per joint {worst:.2e}")
    assert np.abs(r64).reshape(10, -1).max(1).min() > 0
    assert worst <= 3e-5


@pytest.mark.parametrize("coords_kind", ("volume", "cuboids"))
@pytest.mark.parametrize("scale", (1.0, 10.0))
def test_f32_training_step_reference_headroom(scale, coords_kind):
    """The f32 reference chain of the training step stays within 2e-5 per frame of float64
    (the GPU bar is 1e-4 per frame), and its loss within 1e-6."""
    c = cases.train_step_case(scale, cases.train_step_cuboid_frames()[2] if coords_kind == "cuboids" else None)
    l64, g64 = cases.train_step_ref(c)
    l32, g32 = cases.train_step_ref(c, torch.float32)
    worst = max_rel_per(g32, g64, 1).max()
    print(f"scale={scale} {coords_kind}: f32 vs f64 per frame {worst:.2e}, loss {abs(l32 - l64) / abs(l64):.2e}")
    assert worst <= 2e-5
    assert abs(l32 - l64) <= 1e-6 * abs(l64)
    assert (g64[:, :, 5:] == 0).all() and np.abs(g64[:, :, :5]).max() > 0


@pytest.mark.parametrize("n_views", cases.VIEW_COUNTS)
def test_unprojection_geometries_land_on_their_paths(n_views):
    """'lds': every tile's footprints (summed over the views) fit the backward's 1,022 LDS
    slots with the f32-rounding margin of 64, and every axis has a partial tile; 'direct':
    tiles past the budget exist — all of them for 3 views and more."""
    c = cases.unproject_case("lds", n_views)
    assert all(s % t for s, t in zip(c["coords"].shape[1:4], cases.TILE))
    areas = tile_footprints(c["proj"].numpy(), c["coords"].numpy(), 20, 20, cases.TILE)
    assert 0 < areas.sum(1).max() <= cases.LDS_SLOTS - 64
    c = cases.unproject_case("direct", n_views)
    over = tile_footprints(c["proj"].numpy(), c["coords"].numpy(), 64, 64, cases.TILE).sum(1) > cases.LDS_SLOTS + 64
    assert over.all() if n_views >= 3 else over.any()
