"""ORACLE — test infrastructure only.

Seeded inputs and float64 (or f32) CPU references of the backward cases that
tests/test_gpu_backward_shapes.py runs on the GPU and tests/test_backward_refs.py pins on the
CPU: both files build the same tensors from here, so the headroom the CPU file measures (f32
reference against float64) is the headroom of the GPU file's bars.  Every reference is autograd
through oracle/restate_torch.py; the inputs come from mvn_rocm.synth (imported lazily: the
oracle stays importable without the product package).
"""
from __future__ import annotations

import numpy as np
import torch

from . import restate_torch

TILE = (4, 8, 8)            # the unprojection backward's voxel tile (unproject_bwd.hip TX, TY, TZ)
LDS_SLOTS = 1022            # its LDS budget in 16-byte slots (kZero)
VIEW_COUNTS = (1, 2, 3, 5, 7, 8)


class _default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.prev)


def max_rel_per(a, b, keep_dims):
    """max |a - b| / max |b| over the trailing dimensions, one value per element of the first
    `keep_dims` dimensions (per view, per joint, per frame): a slice with a small gradient
    cannot hide behind another's large one.  A slice whose reference is all zero is compared
    absolutely."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    lead = b.shape[:keep_dims]
    a2, b2 = a.reshape(int(np.prod(lead)), -1), b.reshape(int(np.prod(lead)), -1)
    den = np.abs(b2).max(1)
    return (np.abs(a2 - b2).max(1) / np.where(den > 0, den, 1.0)).reshape(lead)


def bf16_round(t):
    """The float32 tensor rounded to bfloat16 and back."""
    return t.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------ unprojection geometry
def unproject_case(path, n_views):
    """Geometry of the view-count tests: B = 2, 6 channels (a partial last channel
    group of 4).  'lds': 20^2 maps on a 24^3 volume cropped to (22, 21, 23) — every axis ends
    in a partial tile and every tile's footprints fit the LDS budget; 'direct': 64^2 maps on a
    16^3 volume — footprints past the budget (every tile for >= 3 views).
    -> dict(feat, proj, coords, conf, gout, heatmap)."""
    from mvn_rocm import synth
    if path == "lds":
        vb = synth.volumetric_batch(2, n_views, channels=6, heatmap=20, volume=24, seed=50 + n_views)
        coords, hm = vb.coords[:, :22, :21, :23].contiguous(), 20
    elif path == "direct":
        vb = synth.volumetric_batch(2, n_views, channels=6, heatmap=64, volume=16, seed=50 + n_views)
        coords, hm = vb.coords, 64
    else:
        raise ValueError(path)
    rng = np.random.default_rng(50 + n_views)
    conf = torch.from_numpy(rng.uniform(0.2, 1.0, (2, n_views, 6)).astype(np.float32))
    gout = torch.randn((2, 6) + tuple(coords.shape[1:4]), generator=torch.Generator().manual_seed(70 + n_views))
    return dict(feat=vb.features, proj=vb.proj, coords=coords, conf=conf, gout=gout, heatmap=hm)


# ------------------------------------------------------------------ 3D soft-argmax
SA_SHAPE = (33, 63, 65)     # 135,135 voxels: 66 pass-1 chunks of 2,048, > 64 * 256 apply threads


def softargmax_case(J=5, channels=None):
    """B = 2 volumes of SA_SHAPE with logits 3 * randn, the training-shaped upstream gradients
    (grad_xyz = 1e-3 * randn, one random cross-entropy voxel per joint).  `channels` > J makes
    the logits a (2, channels, ...) tensor whose first J channels are the case's."""
    from mvn_rocm import synth
    g = torch.Generator().manual_seed(33)
    coords = synth.volumetric_batch(2, channels=1, volume=65, seed=3).coords[:, :33, :63, :65].contiguous()
    logits = 3.0 * torch.randn((2, channels or J) + SA_SHAPE, generator=g)
    grad_xyz = 1e-3 * torch.randn((2, J, 3), generator=g)
    idx = torch.randint(0, int(np.prod(SA_SHAPE)), (2, J), generator=g)
    return dict(logits=logits, coords=coords, grad_xyz=grad_xyz, idx=idx, J=J)


def softargmax_loss(xyz, vols, grad_xyz, idx, mix):
    """The scalar whose gradient the soft-argmax tests take: 'xyz' = sum(xyz * grad_xyz),
    'vol' = mean over (frame, joint) of -log(p[idx] + 1e-6) (VolumetricCELoss's gather), 'full'
    = both.  Works on our op's outputs and on the reference's alike."""
    B, J = xyz.shape[:2]
    loss = 0.0
    if mix in ("full", "xyz"):
        loss = loss + (xyz * grad_xyz.to(xyz)).sum()
    if mix in ("full", "vol"):
        p = vols.reshape(B, J, -1).gather(2, idx.to(vols.device).unsqueeze(-1)).squeeze(-1)
        loss = loss + (-torch.log(p + 1e-6)).sum() / (B * J)
    return loss


def softargmax_ref_grad(logits, coords, softmax, mult, grad_xyz, idx, mix, dtype=torch.float64):
    """d loss / d logits through restate_torch.integrate_tensor_3d_with_coordinates(v * mult)
    in `dtype`, as numpy."""
    v = logits.to(dtype).clone().requires_grad_(True)
    xyz, vols = restate_torch.integrate_tensor_3d_with_coordinates(v * mult, coords.to(dtype), softmax)
    softargmax_loss(xyz, vols, grad_xyz, idx, mix).backward()
    return v.grad.numpy()


def softargmax_ref_explicit(logits, coords, softmax, mult, grad_xyz, grad_vol, dtype=torch.float64):
    """(xyz, vols, d/d logits) with explicit upstream gradients (either may be None)."""
    v = logits.to(dtype).clone().requires_grad_(True)
    xyz, vols = restate_torch.integrate_tensor_3d_with_coordinates(v * mult, coords.to(dtype), softmax)
    outs, grads = [], []
    if grad_xyz is not None:
        outs.append(xyz), grads.append(grad_xyz.to(dtype))
    if grad_vol is not None:
        outs.append(vols), grads.append(grad_vol.to(dtype))
    torch.autograd.backward(outs, grads)
    return xyz.detach().numpy(), vols.detach().numpy(), v.grad.numpy()


def ce_grad_vol(vols, idx):
    """The gradient of mean(-log(p[idx] + 1e-6)) w.r.t. the volumes `vols` (B, J, ...), dense."""
    B, J = vols.shape[:2]
    flat = torch.as_tensor(vols).reshape(B, J, -1).double()
    g = torch.zeros_like(flat)
    p = flat.gather(2, idx.unsqueeze(-1))
    g.scatter_(2, idx.unsqueeze(-1), -1.0 / (p + 1e-6) / (B * J))
    return g.reshape(vols.shape)


# ------------------------------------------------------------------ DLT
def dlt_case(n_views):
    """B = 8 frames x 17 joints (136 threads: three 64-thread blocks, 8 live threads in the
    last); for 4 and 8 views, view 1 of every other frame has zero confidence at every third
    joint."""
    from mvn_rocm import synth
    ab = synth.algebraic_batch(8, n_views, 17, seed=40 + n_views)
    conf = ab.confidences.clone()
    if n_views >= 4:
        conf[::2, 1, ::3] = 0.0
    gout = torch.randn((8, 17, 3), generator=torch.Generator().manual_seed(40 + n_views))
    return dict(proj=ab.proj, points=ab.points, conf=conf, gout=gout)


def dlt_ref_f64(proj, points, conf, gout):
    """(grad_pts, grad_conf or None): float64 autograd of restate_torch.triangulate_batch_of_points."""
    p = points.double().clone().requires_grad_(True)
    c = conf.double().clone().requires_grad_(True) if conf is not None else None
    restate_torch.triangulate_batch_of_points(proj.double(), p, c).backward(gout.double())
    return p.grad.numpy(), (c.grad.numpy() if c is not None else None)


# ------------------------------------------------------------------ the training step
def train_step_case(scale, coords=None):
    """B = 2, 4 views, 8 channels, 5 joints, 20^2 maps, a 24^3 volume (seed 61), features scaled
    by `scale`; keypoints = a random voxel centre + U(-20, 20) mm per joint, validity all ones.
    `coords` replaces the synthetic coordinate volume (the in-kernel-coordinates variant)."""
    from mvn_rocm import synth
    vb = synth.volumetric_batch(2, n_views=4, channels=8, heatmap=20, volume=24, seed=61)
    coords = vb.coords if coords is None else torch.as_tensor(coords, dtype=torch.float32)
    rng = np.random.default_rng(61)
    vox = rng.integers(0, 24, (2, 5, 3))
    centre = coords[torch.arange(2).view(2, 1), vox[..., 0], vox[..., 1], vox[..., 2]]          # (2, 5, 3)
    kps = centre + torch.from_numpy(rng.uniform(-20.0, 20.0, (2, 5, 3)).astype(np.float32))
    return dict(feat=vb.features * scale, proj=vb.proj, coords=coords, kps=kps,
                validity=torch.ones((2, 5, 1)), J=5)


def train_step_cuboid_frames():
    """(base points (2, 3) f64, thetas (2,), the (2, 24, 24, 24, 3) f32 coordinate volume of the
    2,500 mm cuboids around them: restate_np.coord_volumes) of the in-kernel-coordinates
    variant of the training step."""
    from . import restate_np
    rng = np.random.default_rng(61)
    base = rng.uniform(-500, 500, (2, 3)) + np.array([0, 0, 900.0])
    thetas = rng.uniform(0, 2 * np.pi, 2)
    return base, thetas, restate_np.coord_volumes(base, 2500.0, 24, thetas, "coco", False)


def train_step_ref(case, dtype=torch.float64):
    """(loss, grad_feat) of unprojection (softmax) -> channel slice [:J] -> soft-argmax ->
    L1 + 0.01 * VolumetricCELoss through restate_torch in `dtype`."""
    with _default_dtype(dtype):
        f = case["feat"].to(dtype).clone().requires_grad_(True)
        coords = case["coords"].to(dtype)
        vol = restate_torch.unproject_heatmaps(f, case["proj"].to(dtype), coords, "softmax")
        xyz, vols = restate_torch.integrate_tensor_3d_with_coordinates(vol[:, :case["J"]], coords, True)
        kps = case["kps"].to(dtype)
        loss = (xyz - kps).abs().mean() + 0.01 * restate_torch.volumetric_ce_loss(
            coords, vols, kps, case["validity"].to(dtype))
        loss.backward()
        return float(loss.detach()), f.grad.numpy()
