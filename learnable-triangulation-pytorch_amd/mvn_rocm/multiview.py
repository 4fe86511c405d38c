"""Drop-in replacements for the DLT functions of ``mvn/utils/multiview.py``."""
from __future__ import annotations

import torch

from . import _ops


def triangulate_batch_of_points(proj_matricies_batch, points_batch, confidences_batch=None):
    """Confidence-weighted linear triangulation of (B, J) points from N views.

    Reference: ``mvn/utils/multiview.py:162-174`` (+ solver ``:132-159``).
      proj_matricies_batch (B, N, 3, 4), points_batch (B, N, J, 2),
      confidences_batch (B, N, J) or None  ->  (B, J, 3) float32.
    The null vector is computed in float64 (the float32 reference
    SVD itself deviates from float64 by up to ~2e-4 relative).
    """
    if proj_matricies_batch.shape[:2] != points_batch.shape[:2]:   # multiview.py:143
        raise AssertionError("proj_matricies and points must have the same number of views")
    proj = _ops.f32c(proj_matricies_batch)
    pts = _ops.f32c(points_batch)
    conf = None if confidences_batch is None else _ops.f32c(confidences_batch)
    if torch.is_grad_enabled() and (pts.requires_grad or (conf is not None and conf.requires_grad)):
        return DLTFunction.apply(proj, pts, conf)
    return _ops.call(_ops.dlt, proj, pts, conf)


def triangulate_point_from_multiple_views_linear_torch(proj_matricies, points, confidences=None):
    """Single point: proj (N, 3, 4), points (N, 2), confidences (N,) -> (3,).

    Reference: ``mvn/utils/multiview.py:132-159``.
    """
    if len(proj_matricies) != len(points):                          # multiview.py:143
        raise AssertionError("proj_matricies and points must have the same number of views")
    conf = None if confidences is None else confidences.reshape(1, -1, 1)
    return triangulate_batch_of_points(proj_matricies.unsqueeze(0), points.reshape(1, -1, 1, 2), conf)[0, 0]


class DLTFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, proj, pts, conf):
        out = _ops.call(_ops.dlt, proj, pts, conf)
        ctx.save_for_backward(proj, pts, conf)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import _backward
        return _backward.dlt_backward(ctx, grad_out)


# ------------------------------------------------------------------------------- RANSAC
def _tensor(x, device=None):
    """x (tensor, numpy array or a sequence of either) as a detached tensor."""
    if isinstance(x, (list, tuple)) and len(x) and torch.is_tensor(x[0]):
        x = torch.stack(list(x))
    t = x if torch.is_tensor(x) else torch.as_tensor(x)
    t = t.detach()
    return t if device is None else t.to(device)


def calc_reprojection_error_matrix(keypoints_3d, keypoints_2d_list, proj_matricies):
    """Half the pixel distance between every 2D point and the projection of its 3D point.

    Reference: ``mvn/utils/multiview.py:177-184``, same argument order and meaning:
      keypoints_3d (J, 3), keypoints_2d_list (N, J, 2), proj_matricies (N, 3, 4) -> (J, N),
    or all three with a leading batch axis -> (B, J, N).  float32 out, float64 arithmetic.
    """
    X = _tensor(keypoints_3d)
    pts = _tensor(keypoints_2d_list, X.device)
    proj = _tensor(proj_matricies, X.device)
    single = X.dim() == 2
    if single:
        X, pts, proj = X.unsqueeze(0), pts.unsqueeze(0), proj.unsqueeze(0)
    if pts.shape[:2] != proj.shape[:2]:
        raise AssertionError("keypoints_2d_list and proj_matricies must have the same number of views")
    if X.shape[:2] != (pts.shape[0], pts.shape[2]):
        raise AssertionError("keypoints_3d and keypoints_2d_list must have the same number of points")
    out = _ops.call(_ops.reprojection_error, _ops.f32c(X), _ops.f32c(pts), _ops.f32c(proj))
    return out[0] if single else out


def all_view_pairs(n_views, device=None):
    """Every pair a < b of n_views views in lexicographic order, (n_views (n_views - 1) / 2, 2) int32."""
    return torch.triu_indices(n_views, n_views, 1).t().to(torch.int32).contiguous().to(device)


def random_view_pairs(batch_size, n_joints, n_views, n_iters, device, generator=None):
    """n_iters sorted pairs of distinct views per point, drawn uniformly on `device`:
    (batch_size, n_joints, n_iters, 2) int32 (the reference's random.sample(view_set, 2),
    triangulation.py:85)."""
    shape = (batch_size, n_joints, n_iters)
    a = torch.randint(0, n_views, shape, device=device, generator=generator)
    b = torch.randint(0, n_views - 1, shape, device=device, generator=generator)
    b = b + (b >= a).to(b.dtype)
    return torch.stack([torch.minimum(a, b), torch.maximum(a, b)], dim=-1).to(torch.int32)


def triangulate_ransac_batch(proj_matricies_batch, points_batch, *, view_pairs="all", n_iters=10,
                             reprojection_error_epsilon=15, direct_optimization=True, generator=None,
                             return_error=False):
    """RANSAC triangulation of (B, J) points from N views, with Huber refinement.

    Reference: the host loop of ``mvn/models/triangulation.py:54-128``.
      proj_matricies_batch (B, N, 3, 4), points_batch (B, N, J, 2) of any real or integer
      dtype  ->  keypoints_3d (B, J, 3) float32, inliers (B, J, N) bool
      (and, with return_error, the mean reprojection error over the inliers, (B, J) float32).
    view_pairs: 'all' (every pair a < b in lexicographic order: deterministic, n_iters is
    ignored), 'random' (n_iters pairs per point drawn on the device with `generator`), or an
    integer tensor (n_iters, 2) shared by all points or (B, J, n_iters, 2).  A pair with an
    index outside [0, N) or two equal indices is skipped.  Not differentiable (the reference's
    path is numpy): inputs that require grad are detached.
    """
    proj = _tensor(proj_matricies_batch)
    pts = _tensor(points_batch, proj.device)
    if proj.shape[:2] != pts.shape[:2]:                             # triangulation.py:73
        raise AssertionError("proj_matricies and points must have the same number of views")
    B, N, J = pts.shape[:3]
    if N < 2:                                                       # triangulation.py:74
        raise AssertionError("RANSAC triangulation needs at least 2 views")
    if N > 32:
        raise ValueError(f"at most 32 views (got {N}): the inlier set is a 32-bit mask")
    if isinstance(view_pairs, str):
        if view_pairs == "all":
            pairs = all_view_pairs(N, pts.device)
        elif view_pairs == "random":
            if not 1 <= int(n_iters) <= 4096:
                raise ValueError(f"n_iters must be in [1, 4096] (got {n_iters})")
            pairs = random_view_pairs(B, J, N, int(n_iters), pts.device, generator)
        else:
            raise ValueError(f"view_pairs must be 'all', 'random' or an integer tensor (got {view_pairs!r})")
    else:
        pairs = _tensor(view_pairs, pts.device)
        if pairs.dtype.is_floating_point or pairs.dtype.is_complex or pairs.dtype is torch.bool:
            raise TypeError(f"view_pairs must be an integer tensor (got {pairs.dtype})")
        if not ((pairs.dim() == 2 or (pairs.dim() == 4 and tuple(pairs.shape[:2]) == (B, J)))
                and pairs.shape[-1] == 2 and 1 <= pairs.shape[-2] <= 4096):
            raise ValueError(f"view_pairs must be (n_iters, 2) or ({B}, {J}, n_iters, 2) with 1 <= n_iters <= 4096 "
                             f"(got {tuple(pairs.shape)})")
        pairs = pairs.to(torch.int32).contiguous()
    xyz, mask, err = _ops.call(_ops.ransac, _ops.f32c(proj), _ops.f32c(pts), pairs,
                               float(reprojection_error_epsilon), bool(direct_optimization))
    inliers = ((mask.unsqueeze(-1) >> torch.arange(N, device=mask.device, dtype=torch.int32)) & 1).bool()
    return (xyz, inliers, err) if return_error else (xyz, inliers)


def triangulate_ransac(proj_matricies, points, n_iters=10, reprojection_error_epsilon=15, direct_optimization=True,
                       *, view_pairs="random", generator=None):
    """Single point: proj_matricies (N, 3, 4), points (N, 2) -> (point (3,), sorted inlier indices).

    Reference: ``RANSACTriangulationNet.triangulate_ransac`` (``triangulation.py:72-128``) minus
    ``self``; view_pairs and generator as in :func:`triangulate_ransac_batch`.
    """
    if len(proj_matricies) != len(points):                          # triangulation.py:73
        raise AssertionError("proj_matricies and points must have the same number of views")
    if len(points) < 2:                                             # triangulation.py:74
        raise AssertionError("RANSAC triangulation needs at least 2 views")
    proj = _tensor(proj_matricies)
    pts = _tensor(points, proj.device)
    xyz, inliers = triangulate_ransac_batch(proj.unsqueeze(0), pts.reshape(1, -1, 1, 2), view_pairs=view_pairs,
                                            n_iters=n_iters, reprojection_error_epsilon=reprojection_error_epsilon,
                                            direct_optimization=direct_optimization, generator=generator)
    return xyz[0, 0], torch.nonzero(inliers[0, 0]).flatten()
