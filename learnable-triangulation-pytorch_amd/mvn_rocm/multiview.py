"""Drop-in replacements for the DLT functions of ``mvn/utils/multiview.py``."""
from __future__ import annotations

import torch

from . import _lib
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


# ------------------------------------------------------------------------------- algebraic model
# Largest B * J that `fused=None` still sends to the one-launch kernel (csrc/algebraic.hip: one
# block per (b, j), whose one-wave DLT tail keeps the next block off its CU).  The derivable
# rule is one block per CU of the MI355X (256); measured (profiles/time_algebraic.txt, N = 4,
# J = 17, 96^2): faster than the composition by more than the spread up to B = 16 (272 points:
# 50 vs 62 us), slower from B = 64 (1088 points: 126 vs 63 us) — 272 is the largest measured
# size at which the kernel is not slower.
FUSED_MAX_POINTS = 272


def _compose_from_heatmaps(hm, proj, conf, softmax, multiplier, scale_x, scale_y, return_heatmaps, out_dtype):
    """triangulation.py:164-191 from the separate ops (differentiable through their own
    autograd functions)."""
    from . import op
    B, N, J, H, W = hm.shape
    xy, maps = op.integrate_tensor_2d(hm.reshape(B * N, J, H, W), softmax, multiplier=multiplier,
                                      return_heatmaps=return_heatmaps, out_dtype=out_dtype)
    xy = xy.view(B, N, J, 2)
    if conf is None:                                                # triangulation.py:161
        conf = torch.ones((B, N, J), dtype=torch.float32, device=hm.device)
    conf = conf / conf.sum(dim=1, keepdim=True) + 1e-5              # triangulation.py:173-174
    kp2d = torch.stack([xy[..., 0] * scale_x, xy[..., 1] * scale_y], dim=-1)   # triangulation.py:181-183
    xyz = triangulate_batch_of_points(proj, kp2d, conf)
    return xyz, kp2d, (maps.view(B, N, J, H, W) if return_heatmaps else None), conf


def triangulate_from_heatmaps(heatmaps, proj_matricies, confidences=None, *, image_shape, heatmap_multiplier=1.0,
                              heatmap_softmax=True, return_heatmaps=True, out_dtype=None, fused=None):
    """The algebraic model's forward after the backbone, in one call.

    Reference: ``AlgebraicTriangulationNet.forward``, ``mvn/models/triangulation.py:164-191``.
      heatmaps (B, N, J, H, W) — or (B*N, J, H, W), as the backbone returns them, the views then
      taken from proj_matricies — float32 or bfloat16, before the multiplier and the softmax;
      proj_matricies (B, N, 3, 4); confidences (B, N, J) or (B*N, J), raw (``alg_confidences``
      of the backbone), or None for the model without confidences (all ones, ``:161``);
      image_shape (height, width) of the images the projections refer to (``:177``).
    Returns ``forward``'s tuple: keypoints_3d (B, J, 3), keypoints_2d (B, N, J, 2) in image
    pixels, the normalised heatmaps (B, N, J, H, W) in ``out_dtype`` (default: the input's) or
    None with ``return_heatmaps=False``, and the normalised confidences (B, N, J).

    ``fused``: True — one launch (csrc/algebraic.hip); False — the composition of
    ``integrate_tensor_2d``, the normalisation and ``triangulate_batch_of_points``; None
    (default) — the fused kernel up to ``FUSED_MAX_POINTS`` points (B * J), the composition
    above.  Both compute the same 2D points, maps and — given the same confidences — joints bit
    for bit; the fused confidences are summed in view order (torch's sum for N <= 4).  More
    than 32 views always take the composition.  Differentiable with respect to the heatmaps
    and the confidences on both paths.
    """
    from . import op
    hm = heatmaps
    if proj_matricies.dim() != 4 or proj_matricies.shape[2:] != (3, 4):
        raise RuntimeError(f"proj_matricies must be (B, N, 3, 4), got {tuple(proj_matricies.shape)}")
    B, N = proj_matricies.shape[:2]
    if hm.dim() == 4:
        if hm.shape[0] != B * N:
            raise AssertionError("heatmaps and proj_matricies must have the same number of views")
        hm = hm.reshape(B, N, *hm.shape[1:])
    if hm.dim() != 5:
        raise RuntimeError(f"heatmaps must be (B, N, J, H, W) or (B*N, J, H, W), got {tuple(heatmaps.shape)}")
    if hm.shape[:2] != (B, N):                                      # multiview.py:143
        raise AssertionError("heatmaps and proj_matricies must have the same number of views")
    J, H, W = hm.shape[2:]
    in_code = op._dtype_code(hm.dtype)                              # TypeError for anything else
    od = op._dtype_code(out_dtype if out_dtype is not None else hm.dtype)
    if (in_code, od) == (_lib.MVN_DTYPE_F32, _lib.MVN_DTYPE_BF16):
        raise TypeError("float32 heatmaps cannot return bfloat16 maps (bfloat16 in, float32 or bfloat16 out)")
    conf = confidences
    if conf is not None:
        if conf.dim() == 2 and conf.shape[0] == B * N:
            conf = conf.reshape(B, N, conf.shape[1])
        if conf.shape[:2] != (B, N):
            raise AssertionError("confidences and proj_matricies must have the same number of views")
        if tuple(conf.shape) != (B, N, J):
            raise RuntimeError(f"confidences must be {(B, N, J)}, got {tuple(conf.shape)}")
        conf = _ops.f32c(conf)
    hm = hm.contiguous()
    proj = _ops.f32c(proj_matricies)
    scale_x, scale_y = image_shape[1] / W, image_shape[0] / H      # triangulation.py:182-183
    out_t = _ops._CODE_DTYPE[od]
    use_fused = (B * J <= FUSED_MAX_POINTS) if fused is None else bool(fused)
    if not use_fused or N > _ops.ALGEBRAIC_MAX_VIEWS:
        return _compose_from_heatmaps(hm, proj, conf, bool(heatmap_softmax), float(heatmap_multiplier), scale_x,
                                      scale_y, bool(return_heatmaps), out_t)
    args = (hm, proj, conf, bool(heatmap_softmax), float(heatmap_multiplier), float(scale_x), float(scale_y),
            bool(return_heatmaps), od)
    if op._needs_grad(hm, conf):
        xyz, kp2d, maps, cn = AlgebraicFunction.apply(*args)
    else:
        xyz, kp2d, _, cn, maps = _ops.call(_ops.algebraic_triangulate, *args)
    return xyz, kp2d, (maps if return_heatmaps else None), cn


class _Saved:
    """What the existing backward functions read from an autograd context."""

    def __init__(self, saved_tensors, cfg=None, needs_input_grad=()):
        self.saved_tensors, self.cfg, self.needs_input_grad = saved_tensors, cfg, needs_input_grad


class AlgebraicFunction(torch.autograd.Function):
    """autograd surface of triangulate_from_heatmaps' fused path.  No backward kernel of its own:
    the DLT backward (csrc/backward.hip) on the saved image-pixel points and normalised
    confidences, the normalisation's Jacobian and the scale as tensor algebra, and the 2D
    soft-argmax backward on the saved heatmaps and heatmap-pixel points."""

    @staticmethod
    def forward(ctx, hm, proj, conf, softmax, multiplier, scale_x, scale_y, return_maps, out_dtype):
        xyz, kp2d, xy, cn, maps = _ops.call(_ops.algebraic_triangulate, hm, proj, conf, softmax, multiplier,
                                            scale_x, scale_y, return_maps, out_dtype)
        ctx.save_for_backward(hm, proj, conf, xy, kp2d, cn)
        ctx.cfg = (softmax, multiplier, scale_x, scale_y)
        ctx.set_materialize_grads(False)
        return xyz, kp2d, maps, cn

    @staticmethod
    def backward(ctx, g_xyz, g_kp2d, g_maps, g_cn):
        from . import _backward
        hm, proj, conf, xy, kp2d, cn = ctx.saved_tensors
        softmax, multiplier, scale_x, scale_y = ctx.cfg
        want_hm, want_conf = ctx.needs_input_grad[0], conf is not None and ctx.needs_input_grad[2]
        B, N, J, H, W = hm.shape
        # keypoints_3d -> (keypoints_2d, normalised confidences)
        if g_xyz is not None:
            _, g_pts, g_c = _backward.dlt_backward(_Saved((proj, kp2d, cn), needs_input_grad=(False, True, True)), g_xyz)
            g_kp2d = g_pts if g_kp2d is None else g_kp2d + g_pts
            g_cn = g_c if g_cn is None else g_cn + g_c
        g_conf = None
        if want_conf and g_cn is not None:
            # c_u = r_u / s + 1e-5, s = sum_v r_v:  dL/dr_v = g_v / s - sum_u g_u r_u / s^2
            s = conf.sum(dim=1, keepdim=True)
            g_conf = g_cn / s - (g_cn * conf).sum(dim=1, keepdim=True) / (s * s)
        g_hm = None
        if want_hm:
            g_xy = None
            if g_kp2d is not None:
                g_xy = (g_kp2d * g_kp2d.new_tensor([scale_x, scale_y])).reshape(B * N, J, 2)
            gm = g_maps.reshape(B * N, J, H, W) if (g_maps is not None and g_maps.numel() > 0) else None
            if g_xy is None and gm is None:
                g_hm = torch.zeros_like(hm)
            else:
                saved = _Saved((hm.view(B * N, J, H, W), xy.view(B * N, J, 2)), cfg=(softmax, multiplier))
                g_hm = _backward.softargmax2d_backward(saved, g_xy, gm)[0].view_as(hm)
        return g_hm, None, g_conf, None, None, None, None, None, None
